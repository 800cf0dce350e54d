"""GPU: the mutable sparse store (mi355dr_set_sparse / mi355dr_remove_sparse / mi355dr_live_sparse; include/mi355dr.h "sparse
store", "Replace and remove").

The contract: after any sequence of add / set / remove every search, `sparse_df` and the four state stats equal those of a
fresh handle given ONE add_sparse of the current documents.  Every case therefore compares ALL distance bits, ids and NaN / -1
tails with two answers over the current document list: tests/sparse_ref.py as SparseCorpus(current documents), and a fresh
Mi355Index.  No tolerances.  Shapes are those of tests/test_gpu_sparse.py: 1000 Zipf documents over 500 terms, tile 256 (four
tiles), its 37 queries."""

import ctypes

import numpy as np
import pytest

import sparse_ref
import test_gpu_sparse as base_mod
from test_gpu_sparse import N_BASE, RARE, TILE, VOCAB, flat, refused, same, state, zipf_docs

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
BUILD_STATS = ["sparse_full_builds", "sparse_overlay_builds", "sparse_overlay_postings", "sparse_dead_postings"]
EMPTY = (3, 256, 777)


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


@pytest.fixture(scope="module")
def shapes():
    return base_mod.base_docs(), base_mod.base_queries()


class Store:
    """an index and the document list it must answer for"""

    def __init__(self, pkg, docs, **options):
        self.pkg, self.options = pkg, dict({"sparse_tile_docs": TILE}, **options)
        self.docs = [list(d) for d in docs]
        self.ix = self._open()
        if docs:
            self.ix.add_sparse(docs)

    def _open(self):
        ix = self.pkg.Mi355Index(8, "cosine", device=0)
        for key, value in self.options.items():
            ix.set_option(key, value)
        return ix

    def set(self, ids, lists):
        self.ix.set_sparse(ids, lists)
        for i, d in zip(ids, lists):
            self.docs[i] = list(d)

    def remove(self, ids):
        self.ix.remove_sparse(ids)
        for i in ids:
            self.docs[i] = []

    def add(self, lists):
        self.ix.add_sparse(lists)
        self.docs.extend(list(d) for d in lists)

    def builds(self):
        return {s: self.ix.stat(s) for s in BUILD_STATS}

    def check(self, qs, ks=(10,), k1=1.2, b=0.75, bm25=None, device_out=False):
        """searches, df, stats and postings scored against the reference AND a fresh index over the current documents"""
        corpus = sparse_ref.SparseCorpus(self.docs)
        off = self.options.get("row_offset", 0)
        fresh = self._open()
        try:
            fresh.add_sparse(self.docs)
            for k in ks:
                want = sparse_ref.search_weighted(corpus, qs, k, k1, b, row_offset=off)
                s0, f0 = self.ix.stat("sparse_postings_scored"), fresh.stat("sparse_postings_scored")
                got = self.ix.search_sparse(*flat(qs), k, k1=k1, b=b, device_out=device_out)
                scored = self.ix.stat("sparse_postings_scored") - s0
                assert same(got, want), k
                assert same(fresh.search_sparse(*flat(qs), k, k1=k1, b=b), got), k
                assert scored == fresh.stat("sparse_postings_scored") - f0, k
            raw = bm25 if bm25 is not None else [q[0] + q[0][:1] for q in qs]
            got = self.ix.search_bm25(raw, 10, k1=k1, b=b, device_out=device_out)
            assert same(got, sparse_ref.search_bm25(corpus, raw, 10, k1, b, row_offset=off))
            assert same(fresh.search_bm25(raw, 10, k1=k1, b=b), got)
            top = max(corpus.vocab, VOCAB) + 8
            probe = list(range(top)) + [(1 << 20) - 1, 1 << 20, -5]
            assert self.ix.sparse_df(probe).tolist() == [corpus.df(t) for t in probe] == fresh.sparse_df(probe).tolist()
            assert state(self.ix) == [len(self.docs), corpus.n_live, corpus.total_len, corpus.n_postings, corpus.vocab] == state(fresh)
            assert self.ix.live_sparse() == corpus.n_live == fresh.live_sparse()
        finally:
            fresh.close()
        return corpus

    def close(self):
        self.ix.close()


@pytest.fixture()
def store(pkg, shapes):
    s = Store(pkg, shapes[0])
    yield s
    s.close()


def scattered_set(docs):
    """40 documents across the four tiles: the tile edges, the three empty documents revived, every fifth with a term above the
    old vocabulary, every seventh emptied"""
    rng = np.random.default_rng(21)
    ids = [0, 255, 256, 511, 512, 999, 3, 777]
    ids += [int(i) for i in rng.permutation(N_BASE) if i not in ids][:40 - len(ids)]
    lists = zipf_docs(rng, len(ids), VOCAB)
    for j, i in enumerate(ids):
        if j % 5 == 0:
            lists[j] = lists[j] + [600 + j, 600 + j]
        if j % 7 == 6 and i not in EMPTY:
            lists[j] = []
    assert len(set(ids)) == 40 and any(not d for d in lists) and all(lists[ids.index(i)] for i in EMPTY)
    return ids, lists


# ---- 1, 2: a scattered set, answered through the overlay ---------------------------------------------------------------------

def test_scattered_set(store, shapes):
    _, qs = shapes
    store.check(qs)                                        # the base is built
    before = store.builds()
    store.set(*scattered_set(store.docs))
    corpus = store.check(qs, ks=(1, 10, 1024))
    assert corpus.vocab > RARE + 1
    after = store.builds()
    assert after["sparse_overlay_builds"] == before["sparse_overlay_builds"] + 1
    assert after["sparse_full_builds"] == before["sparse_full_builds"]
    assert after["sparse_overlay_postings"] > 0 and after["sparse_dead_postings"] > 0
    assert store.ix.stat("sparse_sets") == 40


def test_threshold_zero_and_large_set_take_the_full_build(pkg, shapes):
    docs, qs = shapes
    s = Store(pkg, docs, sparse_overlay_max_pct=0)
    try:
        s.check(qs)
        before = s.builds()
        s.set(*scattered_set(s.docs))
        s.check(qs, ks=(1, 10, 1024))
        after = s.builds()
        assert after["sparse_full_builds"] == before["sparse_full_builds"] + 1
        assert after["sparse_overlay_builds"] == 0 and after["sparse_overlay_postings"] == 0 and after["sparse_dead_postings"] == 0
    finally:
        s.close()
    s = Store(pkg, docs)                                   # the default threshold: 400 of 1000 documents pass it
    try:
        s.check(qs)
        before = s.builds()
        rng = np.random.default_rng(22)
        ids = rng.permutation(N_BASE)[:400].tolist()
        s.set(ids, zipf_docs(rng, 400, VOCAB))
        s.check(qs, ks=(10, 1024))
        after = s.builds()
        assert after["sparse_full_builds"] == before["sparse_full_builds"] + 1
        assert after["sparse_overlay_builds"] == before["sparse_overlay_builds"] and after["sparse_overlay_postings"] == 0
    finally:
        s.close()


# ---- 3: order of mutations ---------------------------------------------------------------------------------------------------

def test_order_of_mutations(store, shapes):
    _, qs = shapes
    rng = np.random.default_rng(23)
    a, b, c, d = zipf_docs(rng, 4, VOCAB)
    store.check(qs)
    store.set([10, 300], [a, b])
    store.set([10], [c])                                   # the same document twice between searches
    store.set([600], [d])
    store.remove([600])                                    # set then remove
    store.remove([700])
    store.set([700], [a + [VOCAB + 40]])                   # remove then set
    store.check(qs, ks=(10, 1024))
    builds = store.builds()
    store.set([10, 301], [b, c])                           # the overlay is built a second time
    store.check(qs, ks=(10, 1024))
    after = store.builds()
    assert after["sparse_overlay_builds"] == builds["sparse_overlay_builds"] + 1 and after["sparse_full_builds"] == builds["sparse_full_builds"]
    before = state(store.ix), store.builds()
    store.remove([3, 600])                                 # dead documents: a no-op, no build follows
    store.check(qs)
    assert (state(store.ix), store.builds()) == before


# ---- 4: statistics that move -------------------------------------------------------------------------------------------------

def test_statistics_that_move(store, shapes):
    _, qs = shapes
    store.check(qs)
    holders_of = lambda t: [i for i, d in enumerate(store.docs) if t in d]  # noqa: E731
    term = next(t for t in range(300, VOCAB) if holders_of(t) and N_BASE - 1 not in holders_of(t))
    holders = holders_of(term)
    store.remove(holders)
    probe = [([term], [2.0]), ([term, 5], [1.0, 1.0])]
    corpus = store.check(qs + probe, bm25=[[term, 5, 9], [term]])
    assert corpus.df(term) == 0 and store.ix.sparse_df([term])[0] == 0
    d, r = store.ix.search_sparse([term], [2.0], [0, 1], 10)
    assert (r == -1).all() and np.isnan(d).all()
    assert store.ix.stat("sparse_vocab") == RARE + 1
    store.remove([N_BASE - 1])                             # the only document with the largest term
    corpus = store.check(qs)
    assert store.ix.stat("sparse_vocab") == corpus.vocab <= VOCAB
    store.remove(list(range(N_BASE)))                      # N = 0: every line NaN / -1, no division by zero
    corpus = store.check(qs, ks=(10, 1024))
    assert corpus.n_live == 0 and state(store.ix) == [N_BASE, 0, 0, 0, 0]
    d, r = store.ix.search_sparse(*flat(qs), 10)
    assert (r == -1).all() and np.isnan(d).all()
    store.set([500], [[0, 5, 5, VOCAB + 3]])               # one document revived
    store.check(qs + [([5], [1.0])], ks=(10, 1024))
    assert store.ix.live_sparse() == 1


# ---- 5: appends with an overlay ----------------------------------------------------------------------------------------------

def test_appends_with_an_overlay(store, shapes):
    _, qs = shapes
    rng = np.random.default_rng(25)
    store.check(qs)
    before = store.builds()
    store.set([5, 400, 900], zipf_docs(rng, 3, VOCAB))
    store.add(zipf_docs(rng, 49, VOCAB) + [[]])            # 50 documents: the tail rides the overlay
    store.set([N_BASE + 7, N_BASE + 49], [[1, 2, VOCAB + 60], [4, 4]])   # just appended, before any search
    store.check(qs, ks=(10, 1024))
    after = store.builds()
    assert after["sparse_overlay_builds"] == before["sparse_overlay_builds"] + 1
    assert after["sparse_full_builds"] == before["sparse_full_builds"] and after["sparse_overlay_postings"] > 0
    store.add(zipf_docs(rng, 300, VOCAB))                  # past the threshold: a full build
    store.check(qs, ks=(10, 1024))
    last = store.builds()
    assert last["sparse_full_builds"] == after["sparse_full_builds"] + 1 and last["sparse_overlay_postings"] == 0
    assert last["sparse_overlay_builds"] == after["sparse_overlay_builds"] and store.ix.size_sparse() == N_BASE + 350


# ---- 6: ties across the two layouts ------------------------------------------------------------------------------------------

def test_ties_across_the_two_layouts(store, shapes):
    _, qs = shapes
    store.check(qs[:3])
    store.set([900], [store.docs[100]])
    q = [([0], [1.5])]
    store.check(q, ks=(1024,))
    assert store.builds()["sparse_overlay_postings"] > 0
    d, r = store.ix.search_sparse(*flat(q), 1024)
    at = [r[0].tolist().index(i) for i in (100, 511, 512, 640, 900)]   # equal bits: the id decides, base and overlay alike
    assert at == sorted(at) and len({d[0][i].tobytes() for i in at}) == 1


# ---- 7: refusals change nothing ----------------------------------------------------------------------------------------------

def test_refusals_change_nothing(pkg, store, shapes):
    _, qs = shapes
    ix = store.ix
    store.check(qs)
    store.set([8], [[1, 2, 3]])
    store.check(qs)
    probe = list(range(VOCAB + 20))
    before = state(ix), store.builds(), ix.sparse_df(probe).tolist(), ix.stat("sparse_sets")
    want = ix.search_sparse(*flat(qs), 10)
    inv = lambda call: refused(pkg, E_INVALID, call)  # noqa: E731
    inv(lambda: ix.set_sparse([0, N_BASE], [[1], [2]]))                    # id = size
    inv(lambda: ix.set_sparse([-1], [[1]]))
    inv(lambda: ix.set_sparse([4, 9, 4], [[1], [2], [3]]))                 # a repeated id
    inv(lambda: ix.set_sparse([4, 9], [[1], [1 << 20]]))
    inv(lambda: ix.set_sparse([4], [[-1]]))
    refused(pkg, E_UNSUPPORTED, lambda: ix.set_sparse([4, 9], [[1], [7] * 4096]))
    inv(lambda: ix.remove_sparse([N_BASE]))
    inv(lambda: ix.remove_sparse([-1]))
    inv(lambda: ix.remove_sparse([4, 4]))
    # what the Python layer itself refuses is given to the library directly: decreasing offsets, null buffers with n > 0
    lib, h = ix._lib, ix._h
    i64, i32 = ctypes.c_int64, ctypes.c_int32
    ids, terms = (i64 * 2)(4, 9), (i32 * 4)(1, 2, 3, 4)
    assert lib.mi355dr_set_sparse(h, ids, terms, (i64 * 3)(0, 3, 2), 2) == E_INVALID
    assert lib.mi355dr_set_sparse(h, ids, terms, (i64 * 3)(-1, 1, 2), 2) == E_INVALID
    assert lib.mi355dr_set_sparse(h, None, terms, (i64 * 3)(0, 1, 2), 2) == E_INVALID
    assert lib.mi355dr_set_sparse(h, ids, None, (i64 * 3)(0, 1, 2), 2) == E_INVALID
    assert lib.mi355dr_set_sparse(h, ids, terms, None, 2) == E_INVALID
    assert lib.mi355dr_remove_sparse(h, None, 2) == E_INVALID
    assert lib.mi355dr_set_sparse(h, ids, terms, (i64 * 3)(0, 1, 2), -1) == E_INVALID
    with pytest.raises(ValueError):
        ix.set_sparse([1, 2], [[1]])
    with pytest.raises(ValueError):
        ix.set_sparse([1.5], [[1]])
    # n = 0 is fine
    ix.set_sparse([], [])
    ix.remove_sparse([])
    assert lib.mi355dr_set_sparse(h, None, None, None, 0) == 0 and lib.mi355dr_remove_sparse(h, None, 0) == 0
    assert (state(ix), store.builds(), ix.sparse_df(probe).tolist(), ix.stat("sparse_sets")) == before
    assert same(ix.search_sparse(*flat(qs), 10), want)
    store.check(qs)
    # a view refuses; an index without a sparse store has no id to set
    ix.add(np.random.default_rng(1).standard_normal((40, 8)).astype(np.float32))
    with ix.view(row_ids=np.arange(10)) as v:
        inv(lambda: v.set_sparse([0], [[1]]))
        inv(lambda: v.remove_sparse([0]))
        assert v.live_sparse() == 0
    with pkg.Mi355Index(8, "cosine", device=0) as none:
        inv(lambda: none.set_sparse([0], [[1]]))
        inv(lambda: none.remove_sparse([0]))
        assert none.live_sparse() == 0 and none.size_sparse() == 0


# ---- 8: overflow with an overlay ---------------------------------------------------------------------------------------------

def test_overflow_with_an_overlay(pkg, shapes):
    docs, qs = shapes
    s = Store(pkg, docs, sparse_cand_cap=16)
    try:
        s.check(qs)
        s.set(*scattered_set(s.docs))
        s.ix.reset_stats()
        s.check(qs, ks=(10, 1024))
        assert s.ix.stat("sparse_overflows") > 0 and s.ix.stat("sparse_overlay_builds") == 1 and s.builds()["sparse_overlay_postings"] > 0
    finally:
        s.close()


# ---- 9: kernel edges ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", [2048, 8192])
def test_large_tiles_with_an_overlay(pkg, tile):
    rng = np.random.default_rng(tile)
    docs = zipf_docs(rng, 5000, 300, max_len=30)           # three tiles of 2048, one of 8192
    qs = [(rng.choice(300, size=int(rng.integers(1, 12)), replace=False).tolist(), None) for _ in range(11)] + [([0], None)]
    qs = [(t, rng.uniform(0.2, 3.0, size=len(t)).tolist()) for t, _ in qs]
    s = Store(pkg, docs, sparse_tile_docs=tile)
    try:
        s.check(qs)
        ids = [0, 2047, 2048, 4095, 4096, 4999] + rng.integers(1, 4999, size=150).tolist()
        ids = sorted(set(ids))
        lists = zipf_docs(rng, len(ids), 300, max_len=30)
        lists[3], lists[-1] = [], lists[-1] + [310]
        s.set(ids, lists)
        s.add(zipf_docs(rng, 100, 300, max_len=30))
        s.check(qs, ks=(10, 1024))
        assert s.builds()["sparse_overlay_builds"] == 1 and s.builds()["sparse_overlay_postings"] > 0
    finally:
        s.close()


def test_1024_terms_and_1025_queries_with_an_overlay(pkg):
    rng = np.random.default_rng(5)
    docs = [rng.choice(2000, size=int(rng.integers(1, 60)), replace=False).tolist() for _ in range(300)]
    s = Store(pkg, docs)
    try:
        t1024 = rng.choice(2000, size=1024, replace=False).tolist()
        q = [(t1024, rng.uniform(0.1, 2.0, size=1024).tolist()), ([4, 9], [1.0, 1.0])]
        s.check(q, ks=(20,), bm25=[t1024 + t1024])
        ids = rng.permutation(300)[:12].tolist()
        s.set(ids, [rng.choice(2100, size=int(rng.integers(1, 60)), replace=False).tolist() for _ in ids])
        s.set([17], [[4] * 4095 + [9]])                    # tf = 4095 is stored
        s.check(q, ks=(20, 300), bm25=[t1024 + t1024])     # both LDS slice tables are full
        assert s.builds()["sparse_overlay_postings"] > 0
        qs = [(rng.choice(2000, size=int(rng.integers(1, 6)), replace=False).tolist(), None) for _ in range(1025)]
        qs = [(t, [1.0 + 0.001 * j] * len(t)) for j, (t, _) in enumerate(qs)]
        s.check(qs, ks=(7,), bm25=[q[0] for q in qs[:20]])  # B = 1025: two internal blocks
    finally:
        s.close()


def test_device_forms_row_offset_and_parameters(pkg, shapes):
    docs, qs = shapes
    s = Store(pkg, docs, row_offset=5_000_000_000)
    try:
        s.check(qs)
        s.set(*scattered_set(s.docs))                      # local ids, whatever the row_offset
        s.check(qs, ks=(10, 1024), device_out=True)
        assert s.builds()["sparse_overlay_postings"] > 0
        for k1, b in ((0.0, 0.3), (2.0, 0.0), (0.9, 1.0)):
            s.check(qs, k1=k1, b=b)
    finally:
        s.close()


# ---- 10: a seeded sequence ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pct", [None, 100])
def test_seeded_sequence(pkg, pct):
    rng = np.random.default_rng(77)
    s = Store(pkg, zipf_docs(rng, 300, 120, max_len=40), **({} if pct is None else {"sparse_overlay_max_pct": pct}))
    try:
        for step in range(12):
            n = int(rng.integers(1, 21))
            kind = rng.integers(0, 3)
            if kind == 0:
                s.add([d if rng.random() > 0.1 else [] for d in zipf_docs(rng, n, 130, max_len=40)])
            else:
                ids = rng.permutation(len(s.docs))[:n].tolist()
                if kind == 1:
                    s.set(ids, [d if rng.random() > 0.15 else [] for d in zipf_docs(rng, n, 130, max_len=40)])
                else:
                    s.remove(ids)
            qs = [(rng.choice(130, size=int(rng.integers(1, 9)), replace=False).tolist(), None) for _ in range(8)]
            qs = [(t, rng.uniform(-1.0, 3.0, size=len(t)).tolist()) for t, _ in qs]
            s.check(qs, ks=(int(rng.choice([1, 10, 400])),))
        builds = s.builds()
        print(pct, builds)
        if pct == 100:                                     # the first add alone is a full build
            assert builds["sparse_full_builds"] == 1 and builds["sparse_overlay_builds"] >= 1
    finally:
        s.close()


# ---- 11: the dense side is unaffected ----------------------------------------------------------------------------------------

def test_dense_search_is_unaffected(pkg, shapes):
    docs, qs = shapes
    rng = np.random.default_rng(31)
    C = rng.standard_normal((3000, 8)).astype(np.float32)
    Q = rng.standard_normal((9, 8)).astype(np.float32)
    s = Store(pkg, docs)
    try:
        s.ix.add(C)
        d0, r0 = s.ix.search(Q, 10)
        s.check(qs)
        s.set(*scattered_set(s.docs))
        s.remove([1, 2])
        s.check(qs)
        d1, r1 = s.ix.search(Q, 10)
        assert np.array_equal(r0, r1) and d0.tobytes() == d1.tobytes()
        assert len(s.ix) == 3000
    finally:
        s.close()
