"""GPU: sparse search within a listed subset (mi355dr_search_sparse_subset* / mi355dr_search_bm25_subset* /
mi355dr_score_sparse_subset / mi355dr_score_bm25_subset; include/mi355dr.h "sparse store", "Within a listed subset").

Every case compares ALL distance bits, ids and NaN / -1 tails with tests/sparse_subset_ref.py: the unrestricted reference
ranking (k = the whole corpus) with the unlisted documents struck out.  No tolerances.  Every list runs through both paths --
`sparse_subset_pairs_max` = 0 (the filtered tile pass) and 2048 (the pair pass) -- which must equal each other and the
reference.  Shapes are those of tests/test_gpu_sparse.py: 1000 Zipf documents over 500 terms, tile 256 (four tiles, the last
partial), its 37 queries (negative and zero weights among them), plus one document with tf = 4095."""

import ctypes
import math

import numpy as np
import pytest

import sparse_ref
import sparse_subset_ref as ref
import test_gpu_sparse as base_mod
from test_gpu_sparse import N_BASE, TILE, VOCAB, flat, refused, same, state, zipf_docs

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
PATHS = (0, 2048)            # sparse_subset_pairs_max: the tile pass, the pair pass
EDGES = [0, 255, 256, 511, 512, 767, 768, 999]
SUBSET_STATS = ["sparse_subset_searches", "sparse_subset_scores", "sparse_subset_pairs", "sparse_subset_tiles"]


def subset_docs():
    docs = base_mod.base_docs()
    docs[17] = [4] * 4095 + [9]                    # tf = 4095
    return docs


def messy(rng, listed, row_offset=0):
    """the listed local documents as a caller might send them: global ids in random order with duplicates, -1 padding, ids past
    the store and negative ids"""
    ids = [g + row_offset for g in listed] + [listed[0] + row_offset, listed[-1] + row_offset]
    ids += [-1, -1, -7, row_offset - 1, row_offset + N_BASE, row_offset + N_BASE + 5000, -(2 ** 62), 2 ** 62]
    ids = np.array(ids, dtype=np.int64)
    rng.shuffle(ids)
    return ids


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


@pytest.fixture(scope="module")
def base(pkg):
    docs, qs = subset_docs(), base_mod.base_queries()
    corpus = sparse_ref.SparseCorpus(docs)
    ix = pkg.Mi355Index(8, "cosine", device=0)
    ix.set_option("sparse_tile_docs", TILE)
    ix.add_sparse(docs)
    yield ix, corpus, qs
    ix.close()


def both_paths(ix, call):
    """the call through the tile pass and the pair pass: [(result, stats grown by)]"""
    out = []
    for pairs_max in PATHS:
        ix.set_option("sparse_subset_pairs_max", pairs_max)
        before = {s: ix.stat(s) for s in SUBSET_STATS + ["sparse_postings_scored", "sparse_overflows"]}
        got = call()
        out.append((got, {s: ix.stat(s) - v for s, v in before.items()}))
    ix.set_option("sparse_subset_pairs_max", 2048)
    return out


def check_search(ix, corpus, qs, listed_ids, ks=(1, 10, 1024), row_offset=0, device_out=False, k1=1.2, b=0.75):
    n_local = len(ref.local_ids(corpus, listed_ids, row_offset))
    posts = ref.postings_scored(corpus, qs, listed_ids, row_offset)
    for k in ks:
        want = ref.search_weighted_subset(corpus, qs, k, listed_ids, k1, b, row_offset)
        (tile, ts), (pair, ps) = both_paths(ix, lambda: ix.search_sparse_subset(*flat(qs), k, listed_ids, k1=k1, b=b, device_out=device_out))
        assert same(tile, want), k
        assert same(pair, want), k
        # the stats: the path taken, and the postings added do not depend on it
        assert ts["sparse_subset_searches"] == ps["sparse_subset_searches"] == 1
        assert ts["sparse_postings_scored"] == ps["sparse_postings_scored"] == posts, k
        assert ts["sparse_subset_pairs"] == 0 and ps["sparse_subset_tiles"] == 0
        assert ps["sparse_subset_pairs"] == len(qs) * n_local
        assert (ts["sparse_subset_tiles"] > 0) == (n_local > 0)
    return want


# ---- the lists ------------------------------------------------------------------------------------------------------------------

def test_empty_and_single_lists(base):
    ix, corpus, qs = base
    before = state(ix)
    for listed in ([], [-1, -1], [N_BASE, -5]):
        want = check_search(ix, corpus, qs, np.array(listed, dtype=np.int64), ks=(10,))
        assert (want[1] == -1).all()
    for one in (0, 17, 999, 3):                      # 17 holds tf = 4095; 3 has no tokens: it never matches
        want = check_search(ix, corpus, qs, [one], ks=(1, 10))
        assert set(want[1].reshape(-1).tolist()) <= {one, -1} and ((want[1] == one).any() == (one != 3))
    assert state(ix) == before


def test_every_document_equals_the_unrestricted_search(base):
    ix, corpus, qs = base
    every = np.arange(N_BASE, dtype=np.int64)
    for k in (1, 10, 1024):
        s0 = ix.stat("sparse_postings_scored")
        full = ix.search_sparse(*flat(qs), k)
        scored = ix.stat("sparse_postings_scored") - s0
        assert same(full, sparse_ref.search_weighted(corpus, qs, k))
        for got, grown in both_paths(ix, lambda: ix.search_sparse_subset(*flat(qs), k, every)):
            assert same(got, full), k
            assert grown["sparse_postings_scored"] == scored
    check_search(ix, corpus, qs, every, ks=(10,))


def test_tile_edges_and_a_list_inside_one_tile(base):
    ix, corpus, qs = base
    check_search(ix, corpus, qs, EDGES)
    inside = list(range(512, 768, 3))                # confined to tile 2: one tile per launch
    check_search(ix, corpus, qs, inside)
    ix.set_option("sparse_subset_pairs_max", 0)
    for k, cap in ((10, 2048), (10, 16)):
        ix.set_option("sparse_cand_cap", cap)
        t0, o0 = ix.stat("sparse_subset_tiles"), ix.stat("sparse_overflows")
        got = ix.search_sparse_subset(*flat(qs), k, inside)
        assert same(got, ref.search_weighted_subset(corpus, qs, k, inside))
        # the plan in LISTED documents: first min(m, cap), then growing by seen * ratio
        m, ratio = len(inside), min(16, max(1, cap // (2 * k)))
        launches, seen = 1, min(m, cap)
        while seen < m:
            seen, launches = min(m, seen + seen * ratio), launches + 1
        if ix.stat("sparse_overflows") == o0:        # (every piece of an overflowed launch is one more tile)
            assert ix.stat("sparse_subset_tiles") - t0 == launches
        else:
            assert ix.stat("sparse_subset_tiles") - t0 > launches
    ix.set_option("sparse_cand_cap", 2048)
    ix.set_option("sparse_subset_pairs_max", 2048)


def test_every_third_document_and_a_messy_list(base):
    ix, corpus, qs = base
    rng = np.random.default_rng(41)
    check_search(ix, corpus, qs, list(range(0, N_BASE, 3)))
    listed = sorted(rng.choice(N_BASE, size=300, replace=False).tolist() + [3, 256, 777])
    ids = messy(rng, listed)
    want = check_search(ix, corpus, qs, ids)
    assert same(want, ref.search_weighted_subset(corpus, qs, 1024, listed))     # (duplicates, padding and order change nothing)
    assert not ({3, 256, 777} & set(want[1].reshape(-1).tolist()))
    assert (want[1][0] >= 0).sum() == len(set(listed) - {3, 256, 777})          # k greater than the listed matches: tails


def test_row_offset(pkg, base):
    _, corpus, qs = base
    off = 10_000
    rng = np.random.default_rng(42)
    listed = sorted(rng.choice(N_BASE, size=200, replace=False).tolist())
    with pkg.Mi355Index(8, "cosine", device=0) as ix:
        ix.set_option("sparse_tile_docs", TILE)
        ix.set_option("row_offset", off)
        ix.add_sparse(subset_docs())
        want = check_search(ix, corpus, qs, messy(rng, listed, off), ks=(10, 1024), row_offset=off)
        assert want[1][want[1] >= 0].min() >= off                               # global ids in, global ids out
        # local ids are out of range under an offset: nothing is listed
        d, r = ix.search_sparse_subset(*flat(qs), 10, listed[:50])
        assert (r == -1).all() and np.isnan(d).all()
        pool = np.tile(messy(rng, listed[:40], off), (len(qs), 1))
        assert same_block(ix.score_sparse_subset(*flat(qs), pool), ref.score_weighted_subset(corpus, qs, pool, row_offset=off))


# ---- shapes ---------------------------------------------------------------------------------------------------------------------

def test_device_forms_and_parameters(base):
    ix, corpus, qs = base
    listed = list(range(1, N_BASE, 2))
    check_search(ix, corpus, qs, listed, ks=(10, 1024), device_out=True)
    for k1, b in ((0.0, 0.3), (2.0, 0.0)):
        check_search(ix, corpus, qs, listed, ks=(10,), k1=k1, b=b)


def test_bm25_forms_use_the_global_statistics(base):
    ix, corpus, qs = base
    raw = [q[0] + q[0][:1] + [VOCAB + 100] for q in qs]
    listed = list(range(0, N_BASE, 7))
    N = corpus.n_live
    weighted = [(sorted(set(t for t in q if corpus.df(t))), None) for q in raw]
    weighted = [(t, [math.log(1.0 + ((N - corpus.df(x)) + 0.5) / (corpus.df(x) + 0.5)) for x in t]) for t, _ in weighted]
    for k in (10, 1024):
        want = ref.search_weighted_subset(corpus, weighted, k, listed)           # math.log weights from the GLOBAL df
        assert same(ref.search_bm25_subset(corpus, raw, k, listed), want)
        for device_out in (False, True):
            for got, _ in both_paths(ix, lambda: ix.search_bm25_subset(raw, k, listed, device_out=device_out)):
                assert same(got, want)
    pool = np.tile(np.array(listed[:60] + [-1, 3], dtype=np.int64), (len(raw), 1))
    assert same_block(ix.score_bm25_subset(raw, pool), ref.score_weighted_subset(corpus, weighted, pool))
    assert ix.sparse_df([0, 5, VOCAB + 100]).tolist() == [corpus.df(0), corpus.df(5), 0]


def test_1024_terms_and_1025_queries(pkg):
    rng = np.random.default_rng(5)
    docs = [rng.choice(2000, size=int(rng.integers(1, 60)), replace=False).tolist() for _ in range(300)]
    corpus = sparse_ref.SparseCorpus(docs)
    listed = sorted(rng.choice(300, size=120, replace=False).tolist())
    with pkg.Mi355Index(8, "cosine", device=0) as ix:
        ix.set_option("sparse_tile_docs", TILE)
        ix.add_sparse(docs)
        t1024 = rng.choice(2000, size=1024, replace=False).tolist()
        q = [(t1024, rng.uniform(0.1, 2.0, size=1024).tolist()), ([4, 9], [1.0, 1.0])]
        check_search(ix, corpus, q, listed, ks=(20, 300))                        # the slice tables are full; four rounds of pairs
        qs = [(rng.choice(2000, size=int(rng.integers(1, 6)), replace=False).tolist(), None) for _ in range(1025)]
        qs = [(t, [1.0 + 0.001 * j] * len(t)) for j, (t, _) in enumerate(qs)]
        check_search(ix, corpus, qs, listed, ks=(7,))                            # B = 1025: two internal blocks
        pool = rng.integers(-2, 300, size=(1025, 7))
        assert same_block(ix.score_sparse_subset(*flat(qs), pool), ref.score_weighted_subset(corpus, qs, pool))


# ---- overflow of the filtered pass ----------------------------------------------------------------------------------------------

def rising_docs(n=200):
    """equal length, the query term's tf rises with the id: every later document beats every earlier one"""
    return [[1] * (i + 1) + [2] * (n - i) for i in range(n)]


def test_the_rising_store_ranks_by_descending_id():
    corpus = sparse_ref.SparseCorpus(rising_docs())
    d, r = sparse_ref.search_weighted(corpus, [([1], [1.0])], 200)
    assert r[0].tolist() == list(range(199, -1, -1)) and (np.diff(d[0]) > 0).all()


def test_overflow_of_the_filtered_pass(pkg):
    docs = rising_docs()
    corpus = sparse_ref.SparseCorpus(docs)
    qs = [([1], [1.0]), ([2], [1.0]), ([1, 2], [1.0, -0.5])]
    listed = list(range(3, 200, 1))[:160]            # >= 128 listed documents: ranges of 16, 16, 32, 64, ... listed documents
    with pkg.Mi355Index(8, "cosine", device=0) as ix:
        ix.set_option("sparse_tile_docs", TILE)
        ix.set_option("sparse_cand_cap", 16)
        ix.set_option("sparse_subset_pairs_max", 0)
        ix.add_sparse(docs)
        got = ix.search_sparse_subset(*flat(qs), 10, listed)
        assert ix.stat("sparse_overflows") > 0 and ix.stat("sparse_subset_pairs") == 0
        assert same(got, ref.search_weighted_subset(corpus, qs, 10, listed))
        assert got[1][0].tolist() == listed[::-1][:10]
        refused(pkg, E_INVALID, lambda: ix.set_option("sparse_subset_pairs_max", 17))   # above the cap
        ix.set_option("sparse_subset_pairs_max", 16)
        assert same(ix.search_sparse_subset(*flat(qs), 10, listed[:16]), ref.search_weighted_subset(corpus, qs, 10, listed[:16]))
        assert ix.stat("sparse_subset_pairs") == 16 * len(qs)


# ---- a mutated store ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pct", [25, 0])
def test_mutated_store(pkg, base, pct):
    _, _, qs = base
    rng = np.random.default_rng(43)
    docs = subset_docs()
    with pkg.Mi355Index(8, "cosine", device=0) as ix:
        ix.set_option("sparse_tile_docs", TILE)
        ix.set_option("sparse_overlay_max_pct", pct)
        ix.add_sparse(docs)
        ix.search_sparse(*flat(qs[:2]), 5)                                       # the base is built
        moved = sorted(set([0, 255, 256, 999] + rng.choice(N_BASE, size=50, replace=False).tolist()))
        new = zipf_docs(rng, len(moved), VOCAB)
        new[1] = new[1] + [VOCAB + 30]                                           # a term above the base's vocabulary
        ix.set_sparse(moved, new)
        for i, d in zip(moved, new):
            docs[i] = d
        gone = [5, 300, 512, moved[7]]
        ix.remove_sparse(gone)
        for i in gone:
            docs[i] = []
        tail = zipf_docs(rng, 30, VOCAB) + [[]]
        ix.add_sparse(tail)
        docs = docs + tail
        corpus = sparse_ref.SparseCorpus(docs)
        n = len(docs)
        listed = sorted(set(moved[::2] + [moved[1]] + gone + list(range(N_BASE - 5, n)) + rng.choice(n, size=200, replace=False).tolist()))
        builds = ix.stat("sparse_overlay_builds")
        want = check_search(ix, corpus, qs + [([VOCAB + 30], [1.0])], listed, ks=(10, 1024))
        assert ix.stat("sparse_overlay_builds") == builds + (1 if pct else 0)
        assert (ix.stat("sparse_overlay_postings") > 0) == bool(pct)
        assert not (set(gone) & set(want[1].reshape(-1).tolist()))               # a listed removed document never appears
        assert want[1][-1, 0] == moved[1]
        check_search(ix, corpus, qs, moved + gone + [n - 2, n - 1], ks=(10,))    # moved, emptied and appended documents alone
        pool = np.tile(np.array(moved[:20] + gone + [n - 3, n - 1, -1, 1, 2, 2], dtype=np.int64), (len(qs), 1))
        assert same_block(ix.score_sparse_subset(*flat(qs), pool), ref.score_weighted_subset(corpus, qs, pool))


# ---- the score forms ------------------------------------------------------------------------------------------------------------

def same_block(got, want):
    return same((got, np.zeros(got.shape, np.int64)), (want, np.zeros(want.shape, np.int64)))


@pytest.mark.parametrize("m", [1, 7, 300])
def test_score_forms(base, m):
    ix, corpus, qs = base
    rng = np.random.default_rng(m)
    pool = rng.integers(0, N_BASE, size=(len(qs), m))                            # every query its OWN list, duplicates likely at 300
    pool[rng.random(pool.shape) < 0.1] = -1
    pool[0, 0], pool[3, -1] = 3, N_BASE + 4                                      # no tokens; past the store
    if m > 1:
        pool[5, :2] = 17
    before = state(ix), ix.stat("sparse_subset_scores"), ix.stat("sparse_subset_pairs")
    got = ix.score_sparse_subset(*flat(qs), pool)
    want = ref.score_weighted_subset(corpus, qs, pool)
    assert got.shape == (len(qs), m) and same_block(got, want)
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all()                     # no term / none that occurs: nothing matches
    # each value is the unrestricted search's distance for that (query, document)
    fd, fr = ix.search_sparse(*flat(qs), 1024)
    for q in (0, 4, 9):
        of = {r: d for r, d in zip(fr[q].tolist(), fd[q].tolist()) if r >= 0}        # (the tail's -1 is no document)
        for j, g in enumerate(pool[q].tolist()):
            assert (got[q, j] == of[g]) if g in of else np.isnan(got[q, j])
    assert (state(ix), ix.stat("sparse_subset_scores"), ix.stat("sparse_subset_pairs")) == (before[0], before[1] + 1, before[2] + len(qs) * m)


def test_score_forms_without_work(base):
    ix, corpus, qs = base
    assert ix.score_sparse_subset(*flat(qs), np.zeros((len(qs), 0), dtype=np.int64)).shape == (len(qs), 0)
    assert ix.score_sparse_subset([], [], [0], np.zeros((0, 5), dtype=np.int64)).shape == (0, 5)
    assert ix.score_bm25_subset([], np.zeros((0, 5), dtype=np.int64)).shape == (0, 5)
    lib, h = ix._lib, ix._h
    i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert lib.mi355dr_score_sparse_subset(h, None, None, (i32 * 2)(0, 0), 1, 1.2, 0.75, None, 0, None) == 0
    assert lib.mi355dr_score_sparse_subset(h, None, None, None, 0, 1.2, 0.75, None, 4, None) == 0
    assert lib.mi355dr_score_sparse_subset(h, None, None, (i32 * 2)(0, 0), 1, 1.2, 0.75, (i64 * 2)(1, 2), -1, (f64 * 2)()) == E_INVALID
    assert lib.mi355dr_score_sparse_subset(h, None, None, (i32 * 2)(0, 0), 1, 1.2, 0.75, None, 2, (f64 * 2)()) == E_INVALID


# ---- refusals, views ------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(pkg, base):
    ix, corpus, qs = base
    listed = list(range(0, N_BASE, 5))
    want = ix.search_sparse_subset(*flat(qs), 10, listed)
    before = state(ix)
    inv = lambda call: refused(pkg, E_INVALID, call)  # noqa: E731
    inv(lambda: ix.search_sparse_subset(*flat(qs), 0, listed))
    refused(pkg, E_UNSUPPORTED, lambda: ix.search_sparse_subset(*flat(qs), 1025, listed))
    inv(lambda: ix.search_sparse_subset(*flat(qs), 10, listed, k1=-1.0))
    inv(lambda: ix.search_sparse_subset(*flat(qs), 10, listed, k1=float("nan")))
    inv(lambda: ix.search_sparse_subset(*flat(qs), 10, listed, b=1.5))
    inv(lambda: ix.search_bm25_subset([[1, 2]], 10, listed, b=-0.1))
    inv(lambda: ix.search_sparse_subset([4, 4], [1.0, 1.0], [0, 2], 10, listed))                # a repeated term
    inv(lambda: ix.score_sparse_subset([4, 4], [1.0, 1.0], [0, 2], [listed[:3]]))
    inv(lambda: ix.score_sparse_subset([4], [1.0], [0, 1], [listed[:3]], k1=-1.0))
    inv(lambda: ix.set_option("sparse_subset_pairs_max", 2049))
    inv(lambda: ix.set_option("sparse_subset_pairs_max", -1))
    with pytest.raises(ValueError):
        ix.search_sparse_subset(*flat(qs), 10, [1.5])
    with pytest.raises(ValueError):
        ix.score_sparse_subset(*flat(qs), np.zeros((2, 3), dtype=np.int64))
    # m < 0 and a null list with m > 0, given to the library directly
    lib, h = ix._lib, ix._h
    i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    terms, w, off, ids = (i32 * 1)(0), (f64 * 1)(1.0), (i32 * 2)(0, 1), (i64 * 2)(1, 2)
    od, orow = (f64 * 10)(), (i64 * 10)()
    assert lib.mi355dr_search_sparse_subset(h, terms, w, off, 1, 10, 1.2, 0.75, ids, -1, od, orow) == E_INVALID
    assert lib.mi355dr_search_sparse_subset(h, terms, w, off, 1, 10, 1.2, 0.75, None, 2, od, orow) == E_INVALID
    assert lib.mi355dr_search_bm25_subset(h, terms, off, 1, 10, 1.2, 0.75, ids, -1, od, orow) == E_INVALID
    assert lib.mi355dr_search_bm25_subset(h, terms, off, 1, 10, 1.2, 0.75, None, 2, od, orow) == E_INVALID
    assert lib.mi355dr_search_sparse_subset(h, terms, w, off, 1, 10, 1.2, 0.75, None, 0, od, orow) == 0   # m = 0 needs no list
    assert list(orow) == [-1] * 10 and all(x != x for x in od)
    assert state(ix) == before
    assert same(ix.search_sparse_subset(*flat(qs), 10, listed), want)
    assert same(want, ref.search_weighted_subset(corpus, qs, 10, listed))


def test_views_and_empty_stores_answer_nothing(pkg, base):
    _, _, qs = base
    with pkg.Mi355Index(8, "cosine", device=0) as ix:
        for got, _ in both_paths(ix, lambda: ix.search_sparse_subset(*flat(qs), 5, [0, 1, 2])):   # no store at all
            assert (got[1] == -1).all() and np.isnan(got[0]).all()
        assert np.isnan(ix.score_sparse_subset(*flat(qs), np.zeros((len(qs), 3), dtype=np.int64))).all()
        ix.add(np.random.default_rng(1).standard_normal((40, 8)).astype(np.float32))
        ix.add_sparse([[1, 2], [2, 3], []])
        with ix.view(row_ids=np.arange(10)) as v:                                # a view has an empty sparse store: no refusal
            d, r = v.search_sparse_subset([2], [1.0], [0, 1], 4, [0, 1, 2])
            assert (r == -1).all() and np.isnan(d).all()
            d, r = v.search_bm25_subset([[2]], 4, [0, 1, 2])
            assert (r == -1).all() and np.isnan(d).all()
            assert np.isnan(v.score_sparse_subset([2], [1.0], [0, 1], [[0, 1]])).all()
            assert np.isnan(v.score_bm25_subset([[2]], [[0, 1]])).all()
        ix.remove_sparse([0, 1])                                                 # N = 0: every line NaN / -1
        d, r = ix.search_sparse_subset([2], [1.0], [0, 1], 4, [0, 1, 2])
        assert (r == -1).all() and np.isnan(d).all()
        assert np.isnan(ix.score_sparse_subset([2], [1.0], [0, 1], [[0, 1, 2]])).all()


# ---- the service over the real store --------------------------------------------------------------------------------------------

def test_service_over_the_real_store_equals_the_stand_in(pkg, oracle, monkeypatch):
    import autorag_research_amd.service as service
    from helpers import build_golden_stores
    from test_sparse_subset_host import SubsetOracleIndex

    def answers(s, g):
        ids = list(g["ids"])
        text = g["contents"][3]
        within = ids[1::2] + ["no such key"]
        out = [s.bm25_search_by_text(text, 5, within=within), s.bm25_search_by_text(text, 5, within=[ids[3], ids[9]]),
               s.bm25_search_by_text(text, 5, within=[]), s.bm25_search([f"q{i}" for i in range(4)], 4, within=within),
               s.bm25_score_candidates("3 13 57 zzzz", ids + ["no such key"]), s.bm25_score_candidates(text, [ids[3], ids[200]], k1=2.0, b=0.1)]
        return out

    store, g = build_golden_stores()
    real = service.Mi355RetrievalService(lambda: store)
    try:
        got = answers(real, g)
        assert real._unit("chunk").sparse.stat("sparse_subset_searches") == 3 and real._unit("chunk").sparse.stat("sparse_subset_scores") == 2
    finally:
        real.close()
    monkeypatch.setattr(service, "Mi355Index", SubsetOracleIndex)
    store, g = build_golden_stores()
    stand_in = service.Mi355RetrievalService(lambda: store)
    try:
        want = answers(stand_in, g)
    finally:
        stand_in.close()
    assert got == want and len(got[0]) == 5 and len(got[1]) == 2 and got[2] == [] and len(got[4]) == 3
