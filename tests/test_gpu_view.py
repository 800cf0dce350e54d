"""GPU: views (mi355dr_view_create / Mi355Index.view) -- a listed subset of rows or documents gathered on the device into an
index of its own, searched by the ordinary paths, answering under the parent's ids.

The acceptance contract, bit for bit (ids, float8 / fp32 distance bits, NaN positions; NaN payloads are not part of it):
  view.search(Q, k)            == parent.search_subset(Q, k, row_ids) == the oracle over the listed live rows, ids mapped back
  view.search_maxsim(q, off, k) == the oracle over the listed documents with vectors == the host ordering of
                                  parent.maxsim_subset
`_same`, `expect` and `corpus` are the helpers of tests/test_gpu_subset.py."""

import numpy as np
import pytest

from test_gpu_subset import N_SMALL, _same, corpus, expect

pytestmark = pytest.mark.gpu

E_INVALID = -1


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def _nan_tail(res, n_live):
    assert (res[1][:, :n_live] >= 0).all() and (res[1][:, n_live:] == -1).all() and np.isnan(res[0][:, n_live:]).all()


# ---- 1. dims, metrics, k ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", ["cosine", "ip"])
@pytest.mark.parametrize("d", [128, 100, 50], ids=["d128-float4-gather", "d100-float4-gather", "d50-scalar-gather"])
def test_dims_metrics_k(pkg, oracle, d, metric):
    C, Q = corpus(d)
    rng = np.random.default_rng(d)
    ids = rng.choice(N_SMALL, size=1501, replace=False)
    short = rng.choice(N_SMALL, size=37, replace=False)
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(C)
        with idx.view(row_ids=ids) as v, idx.view(row_ids=short) as vs:
            assert v.is_view and not idx.is_view and v.stat("view") == 1 and idx.stat("view") == 0
            assert len(v) == v.live_rows == v.stat("view_rows") == 1501 and len(vs) == 37 and idx.stat("view_rows") == 0
            for B in (24, 40):
                for k in (1, 10, 33, 129, 1024):
                    want = expect(oracle, C, Q[:B], k, ids, metric)
                    _same(v.search(Q[:B], k), want)
                    _same(idx.search_subset(Q[:B], k, ids), want)
                got = vs.search(Q[:B], 50)
                _same(got, expect(oracle, C, Q[:B], 50, short, metric))
                _same(got, idx.search_subset(Q[:B], 50, short))
                _nan_tail(got, 37)


# ---- 2. the screens really run ---------------------------------------------------------------------------------------------

N_BIG, M_BIG = 70_000, 35_000
_BIG = {}


def big_case(oracle):
    """parent of 70 000 rows, a list of 35 000 (above the 16 k and 64 k starter samples: a pass of several chunks); the
    oracle's answers for the three query blocks and both k, computed once"""
    if not _BIG:
        rng = np.random.default_rng(70)
        C = rng.standard_normal((N_BIG, 128)).astype(np.float32)
        Q = rng.standard_normal((200, 128)).astype(np.float32)
        ids = rng.choice(N_BIG, size=M_BIG, replace=False)
        want = {(B, k): expect(oracle, C, Q[:B], k, ids) for B in (1, 40, 200) for k in (10, 100)}
        _BIG.update(C=C, Q=Q, ids=ids, want=want)
    return _BIG["C"], _BIG["Q"], _BIG["ids"], _BIG["want"]


@pytest.fixture(scope="module")
def big_view(pkg, oracle):
    C, Q, ids, want = big_case(oracle)
    with pkg.Mi355Index(128) as idx:
        idx.add(C)
        v = idx.view(row_ids=ids)
    yield v          # (the parent is closed: the view stands alone)
    v.close()


@pytest.mark.parametrize("path", ["auto", "scan"])
@pytest.mark.parametrize("screen_dtype", ["bf16", "i8"])
def test_screens_run_on_a_view(big_view, oracle, screen_dtype, path):
    """B = 1 / 40 (stream kernel), 200 (k_screen_rq for int8, k_screen256c for bf16), and the tile kernel with the stream
    kernel switched off"""
    C, Q, ids, want = big_case(oracle)
    v = big_view
    assert len(v) == M_BIG
    v.set_option("screen_dtype", screen_dtype)
    v.set_option("path", path)
    try:
        for B in (1, 40, 200):
            for k in (10, 100):
                v.reset_stats()
                _same(v.search(Q[:B], k), want[(B, k)])
                if path == "auto":
                    assert v.stat("screen_launches") > 0
                else:
                    assert v.stat("screen_launches") == 0
        if path == "auto":
            v.set_option("screen_stream", 0)
            v.reset_stats()
            _same(v.search(Q[:40], 10), want[(40, 10)])
            assert v.stat("screen_launches") > 0
    finally:
        v.set_option("screen_stream", 1)
        v.set_option("screen_dtype", "auto")
        v.set_option("path", "auto")


# ---- 3. hygiene and row_offset ---------------------------------------------------------------------------------------------

def test_list_hygiene_and_row_offset(pkg, oracle):
    """the dirty list of test_gpu_subset.test_list_hygiene_and_row_offset: shuffled, duplicates, -1 padding, ids below and above
    the shard, +-2^40"""
    C, Q = corpus(100)
    rng = np.random.default_rng(5)
    clean = np.sort(rng.choice(N_SMALL, size=900, replace=False))
    for off in (0, 1000):
        dirty = np.concatenate([clean + off, (clean + off)[::7], np.full(50, -1),
                                [-5, off - 1, N_SMALL + off, N_SMALL + off + 1, 2**40, -2**40]])
        rng.shuffle(dirty)
        with pkg.Mi355Index(100) as idx:
            idx.set_option("row_offset", off)
            idx.add(C)
            want = expect(oracle, C, Q, 33, clean + off, row_offset=off)
            assert want[1].min() >= off
            with idx.view(row_ids=clean + off) as vc, idx.view(row_ids=dirty) as vd:
                assert len(vc) == len(vd) == clean.size
                _same(vc.search(Q, 33), want)
                _same(vd.search(Q, 33), want)
                assert np.array_equal(vd.get_rows(0, clean.size).view(np.uint32), C[clean].view(np.uint32))
            if off:   # ids below row_offset and at or above row_offset + size belong to other shards
                with idx.view(row_ids=np.arange(0, off)) as ve:
                    assert len(ve) == 0 and ve.search(Q[:2], 3)[1].max() == -1


# ---- 4. row classes --------------------------------------------------------------------------------------------------------

def test_row_classes(pkg, oracle):
    """the parent of test_gpu_subset.test_row_classes: irregular rows (0 / NaN / +-inf), > k exact duplicates, removed rows"""
    d, n = 100, 3000
    C, Q = corpus(d, n, 24)
    C, Q = C.copy(), Q.copy()
    rng = np.random.default_rng(8)
    ids = np.sort(rng.choice(n, size=700, replace=False))
    irregular = ids[[3, 90, 91, 400, 699]]
    for v, r in zip((0.0, np.nan, np.inf, -np.inf, 0.0), irregular):
        C[r] = v
    dup = ids[100:160:2]
    C[dup] = Q[0] + 0.01 * rng.standard_normal(d).astype(np.float32)
    unlisted = np.setdiff1d(np.arange(n), ids)
    C[unlisted[unlisted > dup[0]][0]] = C[dup[0]]
    C[unlisted[:3]] = 0.0                                  # irregular rows of the parent that are NOT listed
    loose = ids[[250, 251, 500]]
    C[loose, 0] += 40.0                                    # one dominant component: outside the int8 shadow ("loose"), still ranked
    C[unlisted[10], 1] += 40.0                             # ... and an unlisted one
    shuffled = rng.permutation(ids)
    with pkg.Mi355Index(d) as idx:
        idx.add(C)
        assert idx.stat("irregular_rows") == 8
        with idx.view(row_ids=shuffled) as v:
            assert v.stat("irregular_rows") == 5 and len(v) == 700
            assert 5 + 3 <= v.stat("loose_rows") < idx.stat("loose_rows")       # (irregular rows count as loose too)
            for sd in ("i8", "bf16"):
                v.set_option("screen_dtype", sd)
                _same(v.search(Q, 10), expect(oracle, C, Q, 10, ids))
            v.set_option("screen_dtype", "auto")
            for k in (10, 129, 1024):
                got = v.search(Q, k)
                _same(got, expect(oracle, C, Q, k, ids))
            assert got[1][0, :30].tolist() == dup.tolist()                      # the ties, in the parent's row order
            assert np.isnan(got[0][:, 695:700]).all() and (got[1][:, 700:] == -1).all()
            assert (got[1][:, 695:700] == np.sort(irregular)).all()            # irregular rows last, with NaN, in id order
        live = np.ones(n, bool)
        gone = np.unique(np.concatenate([ids[5:300:3], dup[:4], irregular[:2], rng.choice(n, size=200, replace=False)]))
        idx.remove_rows(gone)
        live[gone] = False
        n_live = int(live[ids].sum())
        with idx.view(row_ids=shuffled) as v:
            assert len(v) == v.live_rows == n_live < 700 and v.stat("dead_rows") == 0
            assert v.stat("irregular_rows") == int(live[irregular].sum()) <= 3
            for k in (10, 129, 1024):
                got = v.search(Q, k)
                _same(got, expect(oracle, C, Q, k, ids, live=live))
                _same(got, idx.search_subset(Q, k, shuffled))
            assert not np.isin(got[1], gone).any()
            assert np.array_equal(v.get_rows(0, n_live).view(np.uint32), C[ids[live[ids]]].view(np.uint32))


# ---- 5. slices -------------------------------------------------------------------------------------------------------------

def test_slices(pkg, oracle):
    """view_slice_rows = 64 with m = 1501: 23 full slices and one of 29 -- the same index as with one slice"""
    C, Q = corpus(100)
    ids = np.random.default_rng(100).choice(N_SMALL, size=1501, replace=False)
    with pkg.Mi355Index(100) as idx:
        idx.add(C)
        with idx.view(row_ids=ids) as whole:
            idx.set_option("view_slice_rows", 64)
            with idx.view(row_ids=ids) as sliced:
                for v in (whole, sliced):
                    assert np.array_equal(v.get_rows(0, 1501).view(np.uint32), C[np.sort(ids)].view(np.uint32))
                    assert v.stat("hbm_bytes_resident") >= 1501 * (100 * 4 + 8)
                for k in (10, 129):
                    want = expect(oracle, C, Q, k, ids)
                    _same(whole.search(Q, k), want)
                    _same(sliced.search(Q, k), want)
                for path, sd in (("scan", "auto"), ("auto", "bf16"), ("auto", "i8")):
                    for v in (whole, sliced):
                        v.set_option("path", path)
                        v.set_option("screen_dtype", sd)
                    _same(sliced.search(Q, 10), whole.search(Q, 10))
                assert sliced.stat("loose_rows") == whole.stat("loose_rows")
        with pytest.raises(pkg.NativeError):
            idx.set_option("view_slice_rows", 31)


# ---- 6. snapshot, read-only, lifetime --------------------------------------------------------------------------------------

def test_snapshot_read_only_lifetime(pkg, oracle):
    d = 100
    C, Q = corpus(d)
    C = C.copy()
    rng = np.random.default_rng(6)
    ids = np.sort(rng.choice(N_SMALL, size=800, replace=False))
    k = 12
    idx = pkg.Mi355Index(d)
    idx.add(C)
    idx.add_multivec(C[:40], np.arange(0, 41, 4))
    v = idx.view(row_ids=ids, doc_ids=np.arange(10))
    before = expect(oracle, C, Q, k, ids)
    _same(v.search(Q, k), before)
    # the parent moves on: an updated listed row (now the best match of Q[0]), a removed one, a compaction
    C2 = C.copy()
    t = int(ids[0] if before[1][0, 0] != ids[0] else ids[1])
    C2[t] = Q[0]
    idx.update_rows([t], C2[[t]])
    after = idx.search_subset(Q, k, ids)
    _same(after, expect(oracle, C2, Q, k, ids))
    assert after[1][0, 0] == t != before[1][0, 0]
    _same(v.search(Q, k), before)
    idx.remove_rows([ids[2], ids[5]])
    idx.compact()
    idx.set_multivec([0], C[:3], [0, 3])
    _same(v.search(Q, k), before)                         # still the old contents under the old ids
    # read-only: every refused call raises INVALID and changes nothing
    one = C[:1]
    qd = np.zeros((1, d))
    refused = [
        lambda: v.add(one), lambda: v.add_device(0, 1), lambda: v.update_rows([0], one), lambda: v.update_rows_device([0], 0),
        lambda: v.remove_rows([0]), lambda: v.compact(), lambda: v.reserve(10), lambda: v.set_option("row_offset", 5),
        lambda: v.add_multivec(C[:2], [0, 2]), lambda: v.add_multivec_device(0, [0, 2]),
        lambda: v.set_multivec([0], C[:2], [0, 2]), lambda: v.set_multivec_device([0], 0, [0, 2]), lambda: v.remove_multivec([0]),
    ]
    ask_parent = [
        lambda: v.search_subset(Q, 3, ids), lambda: v.search_subset_device(0, 1, 3, ids, 0, 0),
        lambda: v.score_subset(Q[:1], [[int(ids[0])]]), lambda: v.maxsim_subset(C[:2], [0, 2], [[0]]),
        lambda: v.gqr_refine(qd, [[int(ids[0])]], [[1.0]], 1, 0.1, 1.0, 0.5),
        lambda: v.gqr_refine_maxsim(qd, [0, 1], [[0]], [[1.0]], 1, 0.1, 1.0, 0.5),
        lambda: v.comm_init(0, 1, b"\0" * 128), lambda: v.comm_init_custom(0, 1, lambda *a: None),
        lambda: v.search_sharded_device(0, 1, 3, 0, 0), lambda: v.view(row_ids=ids),
    ]
    for i, call in enumerate(refused + ask_parent):
        with pytest.raises(pkg.NativeError) as e:
            call()
        assert e.value.code == E_INVALID, i
        assert ("parent" in str(e.value)) == (i >= len(refused)), (i, str(e.value))
    assert len(v) == 800 and v.n_docs() == 10
    _same(v.search(Q, k), before)
    # the stateless entry points stay usable on a view
    z = v.gqr_refine_scores([[0.5, 0.25]], [2], [[0.5, 0.5]], 2, 0.1, 1.0, 0.5)
    assert z.shape == (1, 2) and np.isfinite(z).all()
    # the parent goes first
    idx.close()
    _same(v.search(Q, k), before)
    _same(v.search(Q, 129), expect(oracle, C, Q, 129, ids))
    v.close()


# ---- 7. device forms -------------------------------------------------------------------------------------------------------

def test_device_forms(pkg, oracle):
    C, Q = corpus(128)
    ids = np.arange(1, N_SMALL, 3)
    k, B = 33, len(Q)
    with pkg.Mi355Index(128) as idx:
        idx.add(C)
        with idx.view(row_ids=ids) as v:
            want = expect(oracle, C, Q, k, ids)
            pq, od, orr = v.dev_alloc(Q.nbytes), v.dev_alloc(B * k * 8), v.dev_alloc(B * k * 8)
            v.dev_upload(pq, Q)
            gd, gr = np.empty((B, k)), np.empty((B, k), dtype=np.int64)
            for path in ("auto", "scan"):
                v.set_option("path", path)
                _same(v.search(Q, k), want)
                v.search_device(pq, B, k, od, orr)
                v.dev_download(od, gd)
                v.dev_download(orr, gr)
                _same((gd, gr), want)
                v.dev_upload(orr, np.full((B, k), -7, np.int64))
                ticket = v.search_device_async(pq, B, k, od, orr)
                v.search_wait(ticket)
                v.dev_download(od, gd)
                v.dev_download(orr, gr)
                _same((gd, gr), want)
            for p in (pq, od, orr):
                v.dev_free(p)


def test_sharded_view_at_world_one(pkg, oracle, tmp_path):
    """ShardedSearcher.view with force_pipeline at world 1: pack, all-gather, merge over a view -- the oracle's answer"""
    import torch.distributed as dist

    from autorag_research_amd.sharded import ShardedSearcher

    C, Q = corpus(100)
    ids = np.arange(2, N_SMALL, 5) + 700
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'pg'}", rank=0, world_size=1)
    try:
        s = ShardedSearcher(100, "cosine", device=0)
        s.force_pipeline = True
        s.add_local(C, 700)
        sv = s.view(row_ids=np.concatenate([ids, [5, -1, 2**40]]))
        assert sv.index.is_view and sv.force_pipeline and sv.group is s.group and sv.index is not s.index
        want = expect(oracle, C, Q, 12, ids, row_offset=700)
        _same(sv.search(Q, 12), want)
        _same(sv.search(Q, 12, block=16), want)
        sv.close()
        _same(s.search_subset(Q, 12, ids), want)          # close() released the view only
        s.close()
    finally:
        dist.destroy_process_group()


# ---- 8. edges --------------------------------------------------------------------------------------------------------------

def test_edges(pkg, oracle):
    C, Q = corpus(128)
    with pkg.Mi355Index(128) as idx:
        idx.add(C)
        for ids in (None, np.zeros(0, np.int64), [-1, -9, N_SMALL, N_SMALL + 5, 2**40]):
            with idx.view(row_ids=ids) as v:
                assert v.is_view and len(v) == 0 and v.n_docs() == 0 and v.stat("view_rows") == 0
                d0, r0 = v.search(Q, 5)
                assert np.isnan(d0).all() and (r0 == -1).all()
                dm, rm = v.search_maxsim(C[:3], [0, 3], 4)
                assert np.isnan(dm).all() and (rm == -1).all()
        with idx.view(row_ids=[N_SMALL - 1, 0, 7]) as v:
            got = v.search(Q, 10)
            _same(got, expect(oracle, C, Q, 10, [0, 7, N_SMALL - 1]))
            _nan_tail(got, 3)
        with idx.view(row_ids=np.arange(N_SMALL)) as v:  # every row: the plain index
            _same(v.search(Q, 100), idx.search(Q, 100))
        import ctypes

        from autorag_research_amd._native import check, ptr

        h, one = ctypes.c_void_p(), np.zeros(1, np.int64)
        for args in ((ptr(one, ctypes.c_int64), -1, None, 0), (None, 0, ptr(one, ctypes.c_int64), -1), (None, 1, None, 0),
                     (None, 0, None, 1)):
            with pytest.raises(pkg.NativeError) as e:
                check(idx._h, idx._lib.mi355dr_view_create(idx._h, *args, ctypes.byref(h)))
            assert e.value.code == E_INVALID and not h.value
        with idx.view(row_ids=[1, 2]) as v, pytest.raises(pkg.NativeError) as e:
            v.view(row_ids=[1])
        assert e.value.code == E_INVALID
        _same(idx.search(Q, 10), oracle.topk_search(C, Q, 10))       # the parent is unchanged and usable


# ---- 9. MaxSim -------------------------------------------------------------------------------------------------------------

def _same32(a, b):
    (da, ra), (db, rb) = a, b
    assert np.array_equal(ra, rb)
    assert np.array_equal(np.isnan(da), np.isnan(db))
    ok = ~np.isnan(da)
    assert np.array_equal(da[ok].view(np.uint32), db[ok].view(np.uint32))


def _docs(rng, lens, d):
    out = []
    for t in lens:
        x = rng.standard_normal((int(t), d)).astype(np.float32)
        out.append(x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30))
    return out


def _flat(docs, d):
    tok = np.concatenate(docs, axis=0) if docs else np.zeros((0, d), np.float32)
    return tok.reshape(-1, d), np.concatenate([[0], np.cumsum([t.shape[0] for t in docs])]).astype(np.int64)


def _maxsim_expect(oracle, docs, d, listed, qtok, qoff, k, off=0):
    """oracle top-k over the listed documents that have vectors, ids mapped back to the parent's (global) ids; a query without
    vectors gets what mi355dr_search_maxsim gives it -- nothing (the oracle would score every document 0 for it)"""
    ids = np.unique(np.asarray(listed, np.int64) - off)
    ids = np.array([i for i in ids if 0 <= i < len(docs) and docs[i].shape[0] > 0], np.int64)
    tok, o = _flat([docs[i] for i in ids], d)
    dd, rr = oracle.maxsim_topk(tok, o, qtok, qoff, k)
    none = np.diff(qoff) == 0
    dd[none], rr[none] = np.nan, -1
    return dd, np.where(rr >= 0, (ids[np.maximum(rr, 0)] if ids.size else 0) + off, -1), ids + off


def _subset_order(parent, qtok, qoff, k, ids):
    """the host ordering (distance asc, document asc) of parent.maxsim_subset over `ids`, a query without vectors left empty"""
    B = len(qoff) - 1
    sc = parent.maxsim_subset(qtok, qoff, np.tile(ids, (B, 1)))
    out_d, out_r = np.full((B, k), np.nan, np.float32), np.full((B, k), -1, np.int64)
    for b in range(B):
        ok = ~np.isnan(sc[b])
        order = np.lexsort((ids[ok], sc[b][ok]))[:k]
        out_d[b, :order.size], out_r[b, :order.size] = sc[b][ok][order], ids[ok][order]
    return out_d, out_r


@pytest.mark.parametrize("d", [128, 96])
def test_maxsim(pkg, oracle, d):
    rng = np.random.default_rng(900 + d)
    lens = rng.integers(2, 60, size=300)
    lens[[4, 20, 21, 22, 23, 50, 51, 52]] = [1, 31, 32, 33, 64, 65, 70, 1]
    empty, removed = [7, 100, 299], [0, 21, 150, 151, 298]
    lens[empty] = 0
    docs = _docs(rng, lens, d)
    off = 40
    qlens = [1, 24, 32, 33, 0]
    qtok = np.concatenate(_docs(rng, qlens, d), axis=0)
    qoff = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    listed = np.concatenate([rng.choice(300, size=104, replace=False), empty, removed[:3], [4, 20, 22, 23, 50, 51]]) + off
    dirty = np.concatenate([listed, listed[::5], [-1, -1, off - 1, 300 + off, 2**40, 3]])
    rng.shuffle(dirty)
    assert dirty.size >= 120
    with pkg.Mi355Index(d) as idx:
        idx.set_option("row_offset", off)
        idx.add_multivec(*_flat(docs, d))
        idx.remove_multivec(removed)
        for i in removed:
            docs[i] = docs[i][:0]
        with idx.view(doc_ids=dirty) as v:
            _, _, kept = _maxsim_expect(oracle, docs, d, listed, qtok, qoff, 1, off)
            assert v.n_docs() == v.live_docs() == v.stat("view_docs") == kept.size and len(v) == 0
            assert v.stat("hbm_bytes_resident") > 0
            for screen in (1, 0):
                v.set_option("maxsim_screen", screen)
                for k in (1, 10, 64, 65, 200):
                    want = _maxsim_expect(oracle, docs, d, listed, qtok, qoff, k, off)[:2]
                    got = v.search_maxsim(qtok, qoff, k)
                    _same32(got, want)
                    _same32(got, _subset_order(idx, qtok, qoff, k, kept))
                    assert (got[1][4] == -1).all() and np.isnan(got[0][4]).all()       # the query without vectors ...
                    assert (idx.search_maxsim(qtok, qoff, k)[1][4] == -1).all()        # ... as on the parent
                    if k == 200:
                        assert (got[1][:4, kept.size:] == -1).all() and (got[1][:4, :kept.size] >= off).all()


def test_maxsim_screen_runs_on_a_view(pkg, oracle):
    """3000 of 6000 short documents: the bf16 screen serves the view's queries"""
    d = 128
    rng = np.random.default_rng(6000)
    docs = _docs(rng, rng.integers(1, 12, size=6000), d)
    qlens = [32, 32, 20, 7]
    qtok = np.concatenate(_docs(rng, qlens, d), axis=0)
    qoff = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    listed = rng.choice(6000, size=3000, replace=False)
    with pkg.Mi355Index(d) as idx:
        idx.set_option("view_slice_rows", 4096)            # several token slices
        idx.add_multivec(*_flat(docs, d))
        with idx.view(doc_ids=listed) as v:
            assert v.n_docs() == 3000
            for k in (10, 100):
                _same32(v.search_maxsim(qtok, qoff, k), _maxsim_expect(oracle, docs, d, listed, qtok, qoff, k)[:2])
            assert v.stat("maxsim_screened") > 0 and v.stat("maxsim_fallbacks") == 0


def test_rows_and_documents_in_one_view(pkg, oracle):
    d = 100
    C, Q = corpus(d)
    rng = np.random.default_rng(31)
    docs = _docs(rng, rng.integers(0, 40, size=200), d)
    qlens = [5, 32]
    qtok = np.concatenate(_docs(rng, qlens, d), axis=0)
    qoff = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    rows, listed = rng.choice(N_SMALL, size=500, replace=False), rng.choice(200, size=90, replace=False)
    with pkg.Mi355Index(d) as idx:
        idx.add(C)
        idx.add_multivec(*_flat(docs, d))
        with idx.view(row_ids=rows, doc_ids=listed) as v:
            want_m = _maxsim_expect(oracle, docs, d, listed, qtok, qoff, 10)
            assert len(v) == 500 and v.n_docs() == want_m[2].size
            _same(v.search(Q, 10), expect(oracle, C, Q, 10, rows))
            _same32(v.search_maxsim(qtok, qoff, 10), want_m[:2])
