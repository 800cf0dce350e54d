"""GPU: MaxSim top-k within a listed subset of documents (mi355dr_search_maxsim_subset / Mi355Index.search_maxsim_subset).

The contract, bit for bit (ids, fp32 distance bits, NaN positions; no tolerance anywhere):
  search_maxsim_subset(q, off, k, ids) == the oracle's top-k over the listed documents with vectors (unique, ascending: positions
                                          are in id order, so the tie rule carries over), ids mapped back
                                       == the (distance, document) ordering of maxsim_subset over the list
                                       == view(doc_ids=ids).search_maxsim(q, off, k)
on both paths (option "maxsim_subset_screen" = 1: the list form of the bf16 screen, 0: the exact list path) and with the default.
`_same32`, `_docs`, `_flat`, `_maxsim_expect` and `_subset_order` are the helpers of tests/test_gpu_view.py.

The oracle's answer for one (store, list, queries) is computed once with k = 1024 and cut to every smaller k: the order
(distance, document) is total, so the top-k is a prefix of the top-1024."""

import ctypes

import numpy as np
import pytest

from test_gpu_view import _docs, _flat, _maxsim_expect, _same32, _subset_order

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
N_DOCS = 3000
QLENS = [1, 24, 32, 33, 0]          # the fifth query has no vectors: a NaN / -1 row
KS = (1, 10, 64, 65, 100, 1024)     # 64 / 65: the fast path's boundary; 1024: more than is listed, a NaN tail
# 0, 1, k - 1 and k for every k, 37, 1500, every document
LIST_SIZES = (0, 1, 9, 10, 37, 63, 64, 65, 99, 100, 1023, 1024, 1500, N_DOCS)
LIST_SIZES_WIDE = (0, 1, 9, 10, 37, 1500, N_DOCS)   # d = 200 / 768 (the oracle's time grows with d): k - 1 and k at k = 10


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def _queries(rng, qlens, d):
    qtok = np.concatenate(_docs(rng, qlens, d), axis=0)
    return qtok, np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)


_STORES = {}


def _store_docs(d):
    """3000 documents of 1 .. 70 tokens (1 - 3 blocks), some with exactly 32 and 64, and the five queries"""
    if d not in _STORES:
        rng = np.random.default_rng(4000 + d)
        lens = rng.integers(1, 71, size=N_DOCS)
        lens[[3, 40, 41, 42, 43, 1500, 1501, 2999]] = [1, 31, 32, 33, 64, 65, 70, 32]
        docs = _docs(rng, lens, d)
        _STORES[d] = (docs, *_queries(rng, QLENS, d), {})
    return _STORES[d]


def _listed(d, m):
    """a list of m distinct documents, in no order"""
    return np.random.default_rng(17 * d + m).permutation(N_DOCS)[:m].astype(np.int64)


def _want(oracle, d, m, k):
    docs, qtok, qoff, cache = _store_docs(d)
    if m not in cache:
        cache[m] = _maxsim_expect(oracle, docs, d, _listed(d, m), qtok, qoff, 1024)[:2]
    return cache[m][0][:, :k], cache[m][1][:, :k]


@pytest.fixture(scope="module")
def stores(pkg):
    """one index per dim, built on first use, shared by the tests that only read it"""
    made = {}

    def get(d):
        if d not in made:
            idx = pkg.Mi355Index(d)
            idx.add_multivec(*_flat(_store_docs(d)[0], d))
            made[d] = idx
        return made[d]

    yield get
    for idx in made.values():
        idx.close()


def _set(idx, screen, screen_min=512):
    idx.set_option("maxsim_subset_screen", screen)
    idx.set_option("maxsim_subset_screen_min", screen_min)


# ---- 1. / 2. dims and kernels, both paths and the default, list sizes, k -----------------------------------------------------

@pytest.mark.parametrize("screen", [1, 0, -1], ids=["screen", "exact", "default"])
@pytest.mark.parametrize("d", [128, 96, 200, 768], ids=["d128-unrolled-list-screen", "d96-generic-list-screen",
                                                       "d200-generic-list-screen", "d768-not-screenable"])
def test_dims_lists_k(stores, oracle, d, screen):
    idx = stores(d)
    docs, qtok, qoff, _ = _store_docs(d)
    # the default: from "maxsim_subset_screen_min" listed documents on (set to 1000 here: 1023 and up are screened)
    _set(idx, screen, 1000 if screen < 0 else 512)
    try:
        for m in (LIST_SIZES if d <= 128 else LIST_SIZES_WIDE):
            ids = _listed(d, m)
            screens = d != 768 and m > 0 and (screen == 1 or (screen < 0 and m >= 1000))
            for k in KS:
                idx.reset_stats()
                got = idx.search_maxsim_subset(qtok, qoff, k, ids)
                _same32(got, _want(oracle, d, m, k))
                assert (got[1][4] == -1).all() and np.isnan(got[0][4]).all()
                assert (got[1][:4, :min(k, m)] >= 0).all() and (got[1][:, m:] == -1).all() and np.isnan(got[0][:, m:]).all()
                assert idx.stat("maxsim_subset_searches") == 1 and idx.stat("maxsim_subset_docs") == m
                assert idx.stat("maxsim_subset_fallbacks") == 0
                if screens:
                    assert idx.stat("maxsim_subset_screened") == 4 and idx.stat("maxsim_subset_exact") == 0, (m, k)
                else:
                    assert idx.stat("maxsim_subset_screened") == 0 and idx.stat("maxsim_subset_exact") == (4 if m else 0), (m, k)
    finally:
        _set(idx, -1)


def test_default_threshold(stores, oracle):
    """measured: with nothing set, the list screen serves lists of 512 documents with vectors and more"""
    idx = stores(128)
    docs, qtok, qoff, _ = _store_docs(128)
    for m, screened in ((511, 0), (512, 4), (N_DOCS, 4)):
        ids = _listed(128, m)
        idx.reset_stats()
        _same32(idx.search_maxsim_subset(qtok, qoff, 10, ids), _maxsim_expect(oracle, docs, 128, ids, qtok, qoff, 10)[:2])
        assert idx.stat("maxsim_subset_screened") == screened and idx.stat("maxsim_subset_exact") == 4 - screened, m


@pytest.mark.parametrize("screen", [1, 0], ids=["screen", "exact"])
@pytest.mark.parametrize("B", [1, 5, 17, 37])
def test_batches(stores, oracle, B, screen):
    """more than 4 queries: several groups; more than 16: several passes; at 17 and 37 one query of 130 vectors, more than a
    launch stages at d = 128: it goes in tiles over the list, on either setting"""
    d = 128
    idx = stores(d)
    docs = _store_docs(d)[0]
    rng = np.random.default_rng(50 + B)
    qlens = [QLENS[(b + 1) % 5] for b in range(B)]
    if B >= 17:
        qlens[9] = 130
    qtok, qoff = _queries(rng, qlens, d)
    ids = _listed(d, 1500)
    n_live = sum(1 for n in qlens if n > 0)
    want = _maxsim_expect(oracle, docs, d, ids, qtok, qoff, 100)
    _set(idx, screen)
    try:
        for k in (10, 100):
            idx.reset_stats()
            _same32(idx.search_maxsim_subset(qtok, qoff, k, ids), (want[0][:, :k], want[1][:, :k]))
            n_long = 1 if B >= 17 else 0
            assert idx.stat("maxsim_subset_exact") == (n_long if screen else n_live)
            assert idx.stat("maxsim_subset_screened") == (n_live - n_long if screen else 0)
    finally:
        _set(idx, -1)


def test_long_documents_cooperative_rescore(pkg, oracle):
    """150 documents of 1050 tokens (33 blocks): the candidates of the list screen are re-scored one workgroup per document"""
    d = 128
    rng = np.random.default_rng(33)
    docs = _docs(rng, [1050] * 150, d)
    qtok, qoff = _queries(rng, QLENS, d)
    ids = rng.permutation(150)[:100].astype(np.int64)
    want = _maxsim_expect(oracle, docs, d, ids, qtok, qoff, 100)
    with pkg.Mi355Index(d) as idx:
        idx.add_multivec(*_flat(docs, d))
        for screen in (1, 0):
            _set(idx, screen)
            for k in (10, 65, 100):
                idx.reset_stats()
                _same32(idx.search_maxsim_subset(qtok, qoff, k, ids), (want[0][:, :k], want[1][:, :k]))
                assert idx.stat("maxsim_subset_screened") == (4 if screen else 0)


# ---- 3. the three equalities -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("screen", [1, 0], ids=["screen", "exact"])
def test_three_equalities(stores, oracle, screen):
    d = 128
    idx = stores(d)
    docs, qtok, qoff, _ = _store_docs(d)
    ids = _listed(d, 1500)
    _set(idx, screen)
    try:
        with idx.view(doc_ids=ids) as v:
            for k in (10, 100):
                got = idx.search_maxsim_subset(qtok, qoff, k, ids)
                _same32(got, _want(oracle, d, 1500, k))
                _same32(got, _subset_order(idx, qtok, qoff, k, np.sort(ids)))
                _same32(got, v.search_maxsim(qtok, qoff, k))
    finally:
        _set(idx, -1)


# ---- 4. list hygiene ---------------------------------------------------------------------------------------------------------

def test_list_hygiene_row_offset_removed_revived(pkg, oracle):
    d = 96
    rng = np.random.default_rng(904)
    lens = rng.integers(2, 60, size=300)
    empty, removed = [7, 100, 299], [0, 21, 150, 151, 298]
    lens[empty] = 0                                             # documents added without vectors
    docs = _docs(rng, lens, d)
    off = 40
    qtok, qoff = _queries(rng, QLENS, d)
    listed = np.concatenate([rng.choice(300, size=104, replace=False), empty, removed[:3]]) + off
    dirty = np.concatenate([listed, listed[::5], [-1, -1, -7, off - 1, 300 + off, 2**40, 3]])   # duplicates, padding, out of range
    rng.shuffle(dirty)
    with pkg.Mi355Index(d) as idx:
        idx.set_option("row_offset", off)
        idx.add_multivec(*_flat(docs, d))
        idx.remove_multivec(removed)
        kept_docs = [t if i not in removed else t[:0] for i, t in enumerate(docs)]
        for screen in (1, 0):
            _set(idx, screen)
            for k in (10, 200):
                want = _maxsim_expect(oracle, kept_docs, d, listed, qtok, qoff, k, off)
                idx.reset_stats()
                got = idx.search_maxsim_subset(qtok, qoff, k, dirty)
                _same32(got, want[:2])
                assert idx.stat("maxsim_subset_docs") == want[2].size
                _same32(got, idx.search_maxsim_subset(qtok, qoff, k, want[2]))     # the clean list: the order never matters
                assert (got[1][:4, :min(k, want[2].size)] >= off).all()
            # a list with only documents without vectors: nothing
            none = idx.search_maxsim_subset(qtok, qoff, 10, np.array(empty + removed) + off)
            assert (none[1] == -1).all() and np.isnan(none[0]).all()
        # revived: the removed documents take vectors again and are found again
        new = _docs(rng, [5, 40, 33], d)
        idx.set_multivec(removed[:3], *_flat(new, d))
        for i, t in zip(removed[:3], new):
            kept_docs[i] = t
        for screen in (1, 0):
            _set(idx, screen)
            want = _maxsim_expect(oracle, kept_docs, d, listed, qtok, qoff, 200, off)
            got = idx.search_maxsim_subset(qtok, qoff, 200, dirty)
            _same32(got, want[:2])
            assert set(np.array(removed[:3]) + off) <= set(got[1][0].tolist())


# ---- 5. ties -----------------------------------------------------------------------------------------------------------------

def test_ties_lower_id_wins(pkg, oracle):
    d = 128
    rng = np.random.default_rng(5)
    docs = _docs(rng, rng.integers(1, 40, size=400), d)
    same = [390, 12, 200, 77, 13]
    for i in same:
        docs[i] = docs[12]                  # one document under five ids
    qtok, qoff = _queries(rng, [7, 32], d)
    qtok = np.concatenate([docs[12], qtok])  # the first query IS that document: it is every copy's best match
    qoff = np.concatenate([[0], qoff + docs[12].shape[0]]).astype(np.int32)
    ids = np.concatenate([same, rng.choice(400, size=150, replace=False)])
    with pkg.Mi355Index(d) as idx:
        idx.add_multivec(*_flat(docs, d))
        for screen in (1, 0):
            _set(idx, screen)
            for k in (3, 10, 100):
                got = idx.search_maxsim_subset(qtok, qoff, k, ids)
                _same32(got, _maxsim_expect(oracle, docs, d, ids, qtok, qoff, k)[:2])
                assert got[1][0, :min(k, 5)].tolist() == sorted(same)[:k]
                assert len(set(got[0][0, :min(k, 5)].view(np.uint32).tolist())) == 1


# ---- 6. overflow -------------------------------------------------------------------------------------------------------------

def test_overflow_falls_back_to_the_exact_list_path(pkg, oracle):
    """20 000 copies of one 8-token document, all listed: more than the 8192 candidates a list holds inside the band"""
    d, n = 128, 20_000
    rng = np.random.default_rng(6)
    one = _docs(rng, [8], d)[0]
    tok, off = np.tile(one, (n, 1)), np.arange(n + 1, dtype=np.int64) * 8
    qtok, qoff = _queries(rng, [32, 5], d)
    ids = np.arange(n, dtype=np.int64)
    with pkg.Mi355Index(d) as idx:
        idx.add_multivec(tok, off)
        _set(idx, 1)
        idx.reset_stats()
        got = idx.search_maxsim_subset(qtok, qoff, 10, ids)
        rd, rr = oracle.maxsim_topk(tok, off, qtok, qoff, 10)
        _same32(got, (rd, rr))
        assert idx.stat("maxsim_subset_fallbacks") == 2 and idx.stat("maxsim_subset_exact") == 2
        assert idx.stat("maxsim_subset_screened") == 0 and idx.stat("maxsim_fallbacks") == 0


# ---- 7. a store with a non-finite token ----------------------------------------------------------------------------------------

def test_non_finite_store_takes_the_exact_path(pkg, oracle):
    d = 128
    rng = np.random.default_rng(7)
    docs = _docs(rng, rng.integers(1, 40, size=500), d)
    docs[30] = docs[30].copy()
    docs[30][0, 3] = np.inf
    qtok, qoff = _queries(rng, QLENS, d)
    ids = np.concatenate([[30], rng.choice(500, size=200, replace=False)])
    with pkg.Mi355Index(d) as idx:
        idx.add_multivec(*_flat(docs, d))
        _set(idx, 1)
        idx.reset_stats()
        got = idx.search_maxsim_subset(qtok, qoff, 10, ids)
        _same32(got, _maxsim_expect(oracle, docs, d, ids, qtok, qoff, 10)[:2])
        assert idx.stat("maxsim_subset_screened") == 0 and idx.stat("maxsim_subset_exact") == 4


# ---- 8. errors and refusals --------------------------------------------------------------------------------------------------

def test_errors_and_refusals(stores, pkg, oracle):
    d = 128
    idx = stores(d)
    _, qtok, qoff, _ = _store_docs(d)
    L, h = idx._lib, idx._h
    f32p, i32p, i64p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    ids = np.arange(50, dtype=np.int64)
    out_d, out_r = np.zeros((5, 1025), np.float32), np.zeros((5, 1025), np.int64)

    def call(k, ids_p, m, B=5):
        return L.mi355dr_search_maxsim_subset(h, qtok.ctypes.data_as(f32p), qoff.ctypes.data_as(i32p), B, k, ids_p, m,
                                              out_d.ctypes.data_as(f32p), out_r.ctypes.data_as(i64p))

    assert call(10, ids.ctypes.data_as(i64p), -1) == E_INVALID
    assert call(10, None, 5) == E_INVALID
    assert call(0, ids.ctypes.data_as(i64p), 50) == E_INVALID
    assert call(1025, ids.ctypes.data_as(i64p), 50) == E_UNSUPPORTED
    bad = qoff.copy()
    bad[2] = bad[1] - 1
    assert L.mi355dr_search_maxsim_subset(h, qtok.ctypes.data_as(f32p), bad.ctypes.data_as(i32p), 5, 10, ids.ctypes.data_as(i64p),
                                          50, out_d.ctypes.data_as(f32p), out_r.ctypes.data_as(i64p)) == E_INVALID
    assert call(10, ids.ctypes.data_as(i64p), 50, B=0) == 0
    assert call(10, None, 0) == 0 and (out_r.reshape(-1)[:50] == -1).all() and np.isnan(out_d.reshape(-1)[:50]).all()
    with idx.view(doc_ids=ids) as v:
        with pytest.raises(pkg.NativeError) as e:
            v.search_maxsim_subset(qtok, qoff, 10, ids)
        assert e.value.code == E_INVALID and "parent" in str(e.value)
    _same32(idx.search_maxsim_subset(qtok, qoff, 10, _listed(d, 37)), _want(oracle, d, 37, 10))   # the parent is still usable


# ---- 9. the _device form -----------------------------------------------------------------------------------------------------

MS_STATS = ("maxsim_screened", "maxsim_candidates", "maxsim_fallbacks", "maxsim_screen_cols", "maxsim_packed_launches",
            "maxsim_screen_launches", "maxsim_exact_launches")


@pytest.mark.parametrize("screen", [1, 0], ids=["screen", "exact"])
def test_device_form_and_the_neighbours_are_undisturbed(stores, oracle, screen):
    d, k = 128, 10
    idx = stores(d)
    docs, qtok, qoff, _ = _store_docs(d)
    ids = _listed(d, 1500)
    B = len(qoff) - 1
    tiled = np.tile(np.sort(ids)[:64], (B, 1))
    _set(idx, screen)
    q_dev, d_dev, r_dev = idx.dev_alloc(qtok.nbytes), idx.dev_alloc(B * k * 4), idx.dev_alloc(B * k * 8)
    try:
        before = idx.search_maxsim(qtok, qoff, k), idx.maxsim_subset(qtok, qoff, tiled)
        idx.reset_stats()
        idx.search_maxsim(qtok, qoff, k)
        stats = {s: idx.stat(s) for s in MS_STATS}
        host = idx.search_maxsim_subset(qtok, qoff, k, ids)
        idx.dev_upload(q_dev, qtok)
        idx.search_maxsim_subset_device(q_dev, qoff, k, ids, d_dev, r_dev)
        got_d, got_r = np.empty((B, k), np.float32), np.empty((B, k), np.int64)
        idx.dev_download(d_dev, got_d)
        idx.dev_download(r_dev, got_r)
        _same32((got_d, got_r), host)
        _same32(host, _want(oracle, d, 1500, k))
        assert {s: idx.stat(s) for s in MS_STATS} == stats            # the subset calls moved none of them
        assert idx.stat("maxsim_subset_searches") == 2
        _same32(idx.search_maxsim(qtok, qoff, k), before[0])
        after = idx.maxsim_subset(qtok, qoff, tiled)
        assert np.array_equal(np.isnan(after), np.isnan(before[1]))
        assert np.array_equal(after[~np.isnan(after)].view(np.uint32), before[1][~np.isnan(before[1])].view(np.uint32))
    finally:
        for p in (q_dev, d_dev, r_dev):
            idx.dev_free(p)
        _set(idx, -1)
