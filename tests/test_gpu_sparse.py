"""GPU: the sparse store (mi355dr_add_sparse / mi355dr_search_sparse* / mi355dr_search_bm25*; include/mi355dr.h "sparse store").

Every case compares ALL B x k distances bit for bit, all ids and the NaN / -1 tails with tests/sparse_ref.py (numpy float64,
one operation per operation of the contract).  Shapes are small: tile 256 makes 1000 documents cross four LDS tiles."""

import math

import numpy as np
import pytest

import sparse_ref

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
N_BASE, VOCAB, TILE = 1000, 500, 256
RARE = VOCAB + 7          # occurs only in the last document
UNSEEN = [VOCAB + 100, VOCAB + 101, (1 << 20) - 1]
STATE_STATS = ["sparse_docs", "sparse_total_len", "sparse_postings", "sparse_vocab"]


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def same(got, want):
    """distances bit for bit (NaN equals NaN, -0.0 differs from +0.0), ids exactly"""
    (gd, gr), (wd, wr) = got, want
    return (gd.shape == wd.shape and np.array_equal(gr, wr)
            and np.array_equal(np.ascontiguousarray(gd).view(np.uint64) | (np.isnan(gd) * np.uint64(0xFFFFFFFFFFFFFFFF)),
                               np.ascontiguousarray(wd).view(np.uint64) | (np.isnan(wd) * np.uint64(0xFFFFFFFFFFFFFFFF))))


def zipf_docs(rng, n, vocab, max_len=200):
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    return [rng.choice(vocab, size=int(rng.integers(1, max_len + 1)), p=p).tolist() for _ in range(n)]


def base_docs():
    rng = np.random.default_rng(11)
    docs = zipf_docs(rng, N_BASE, VOCAB)
    for d in docs:
        d[0] = 0                                   # term 0 is in every document
    for i in (3, 256, 777):
        docs[i] = []                               # stored, take an id, never match
    docs[511] = docs[512] = docs[640] = list(docs[100])   # identical documents: equal bits, the id decides
    docs[N_BASE - 1] = docs[N_BASE - 1] + [RARE, RARE]
    return docs


def base_queries():
    """37 queries as (terms, weights): 1 .. 30 distinct terms, an empty one, an all-unseen one, zero / negative weights"""
    rng = np.random.default_rng(12)
    qs = []
    for j in range(37):
        terms = rng.choice(VOCAB, size=int(rng.integers(1, 31)), replace=False)
        rng.shuffle(terms)                         # any order: the library sorts
        qs.append((terms.tolist(), rng.uniform(0.1, 4.0, size=len(terms)).tolist()))
    qs[0] = ([0], [1.5])                           # every document with tokens matches
    qs[1] = ([], [])
    qs[2] = (list(UNSEEN), [1.0, 2.0, 3.0])
    qs[3] = ([0, 5, 17, 2], [0.0, -0.0, 0.0, 0.0])             # score +0.0: distance -0.0, still a match
    qs[4] = ([1, 0, 9, 30], [-1.0, 0.5, -2.5, 0.0])            # scores below zero still match
    qs[5] = ([RARE, UNSEEN[0]], [2.0, 1.0])                    # one match: the last document
    qs[6] = ([RARE, 0], [1e30, -1e30])
    return qs


def flat(qs):
    terms = [t for q in qs for t in q[0]]
    weights = [w for q in qs for w in q[1]]
    offsets = np.concatenate([[0], np.cumsum([len(q[0]) for q in qs])]).astype(np.int64)
    return terms, weights, offsets


@pytest.fixture(scope="module")
def base(pkg):
    docs, qs = base_docs(), base_queries()
    corpus = sparse_ref.SparseCorpus(docs)
    want = {k: sparse_ref.search_weighted(corpus, qs, k) for k in (1, 10, 1024)}
    for d, r in want.values():
        d.setflags(write=False)
        r.setflags(write=False)
    ix = pkg.Mi355Index(8, "cosine", device=0)
    ix.set_option("sparse_tile_docs", TILE)
    ix.add_sparse(docs)
    yield ix, corpus, qs, want
    ix.close()


@pytest.mark.parametrize("k", [1, 10, 1024])
def test_base_case(base, k):
    ix, corpus, qs, want = base
    got = ix.search_sparse(*flat(qs), k)
    assert same(got, want[k])
    wd, wr = want[k]
    if k == 1024:
        assert (wr[0] >= 0).sum() == N_BASE - 3 and (wr[1] == -1).all() and (wr[2] == -1).all()
        assert np.signbit(wd[3][wr[3] >= 0]).all() and (wd[3][wr[3] >= 0] == 0).all()      # -0.0 distances, id order
        assert wr[5].tolist()[:2] == [N_BASE - 1, -1]
        at = [wr[0].tolist().index(i) for i in (100, 511, 512, 640)]                         # equal bits: the id decides
        assert at == sorted(at) and len({wd[0][i].tobytes() for i in at}) == 1


def test_other_parameters(base):
    ix, corpus, qs, _ = base
    for k1, b in ((0.0, 0.3), (2.0, 0.0), (0.9, 1.0)):
        assert same(ix.search_sparse(*flat(qs), 10, k1=k1, b=b), sparse_ref.search_weighted(corpus, qs, 10, k1, b))


@pytest.mark.parametrize("n", [255, 256, 257, 515])
def test_tile_edges(pkg, n):
    rng = np.random.default_rng(n)
    docs = zipf_docs(rng, n, 60, max_len=40)
    docs[n - 1] = docs[n - 1] + [70]
    qs = [(rng.choice(60, size=int(rng.integers(1, 8)), replace=False).tolist(), None) for _ in range(9)] + [([70, 0], None)]
    qs = [(t, rng.uniform(0.5, 2.0, size=len(t)).tolist()) for t, _ in qs]
    corpus = sparse_ref.SparseCorpus(docs)
    with pkg.Mi355Index(8, "cosine", device=0) as ix:
        ix.set_option("sparse_tile_docs", TILE)
        ix.add_sparse(docs)
        for k in (3, n):
            assert same(ix.search_sparse(*flat(qs), k), sparse_ref.search_weighted(corpus, qs, k))


def state(ix):
    return [ix.size_sparse()] + [ix.stat(s) for s in STATE_STATS]


def refused(pkg, code, call):
    with pytest.raises(pkg.NativeError) as e:
        call()
    assert e.value.code == code


def test_shape_limits(pkg):
    rng = np.random.default_rng(5)
    docs = [rng.choice(2000, size=int(rng.integers(1, 60)), replace=False).tolist() for _ in range(300)]
    docs[17] = [4] * 4095 + [9]                    # tf = 4095 is stored
    corpus = sparse_ref.SparseCorpus(docs)
    with pkg.Mi355Index(8, "cosine", device=0) as ix:
        ix.set_option("sparse_tile_docs", TILE)
        ix.add_sparse(docs)
        before = state(ix)
        # 1024 distinct terms in one query; 1025 are refused
        t1024 = rng.choice(2000, size=1024, replace=False).tolist()
        q = [(t1024, rng.uniform(0.1, 2.0, size=1024).tolist()), ([4, 9], [1.0, 1.0])]
        assert same(ix.search_sparse(*flat(q), 20), sparse_ref.search_weighted(corpus, q, 20))
        t1025 = rng.choice(2000, size=1025, replace=False).tolist()
        refused(pkg, E_UNSUPPORTED, lambda: ix.search_sparse(t1025, [1.0] * 1025, [0, 1025], 5))
        refused(pkg, E_UNSUPPORTED, lambda: ix.search_bm25([t1025], 5))
        assert same(ix.search_bm25([t1024 + t1024], 5), sparse_ref.search_bm25(corpus, [t1024], 5))   # repeats count once
        # tf = 4096 is refused and nothing changes, whatever else the call holds
        refused(pkg, E_UNSUPPORTED, lambda: ix.add_sparse([[1, 2], [7] * 4096, [3]]))
        refused(pkg, E_INVALID, lambda: ix.add_sparse([[1, 2], [1 << 20]]))
        refused(pkg, E_INVALID, lambda: ix.add_sparse([[-1]]))
        assert state(ix) == before
        # B = 1025: two internal blocks
        qs = [(rng.choice(2000, size=int(rng.integers(1, 6)), replace=False).tolist(), None) for _ in range(1025)]
        qs = [(t, [1.0 + 0.001 * j] * len(t)) for j, (t, _) in enumerate(qs)]
        assert same(ix.search_sparse(*flat(qs), 7), sparse_ref.search_weighted(corpus, qs, 7))
        assert state(ix) == before


def test_invalid_arguments_leave_the_store_unchanged(base, pkg):
    ix, corpus, qs, want = base
    before = state(ix)
    inv = lambda call: refused(pkg, E_INVALID, call)  # noqa: E731
    inv(lambda: ix.search_sparse([1, 2, 1], [1.0, 1.0, 1.0], [0, 3], 5))              # a repeated term
    inv(lambda: ix.search_sparse([1, 2], [1.0, float("nan")], [0, 2], 5))
    inv(lambda: ix.search_sparse([1, 2], [1.0, float("inf")], [0, 2], 5))
    inv(lambda: ix.search_sparse([1, 2], [1.0, 2e30], [0, 2], 5))
    inv(lambda: ix.search_sparse([1, 1 << 20], [1.0, 1.0], [0, 2], 5))
    inv(lambda: ix.search_sparse([-1], [1.0], [0, 1], 5))
    inv(lambda: ix.search_sparse([1], [1.0], [0, 1], 0))
    for k1, b in ((-0.1, 0.5), (float("inf"), 0.5), (float("nan"), 0.5), (1.2, -0.01), (1.2, 1.01), (1.2, float("nan"))):
        inv(lambda: ix.search_sparse([1], [1.0], [0, 1], 5, k1=k1, b=b))
        inv(lambda: ix.search_bm25([[1]], 5, k1=k1, b=b))
    refused(pkg, E_UNSUPPORTED, lambda: ix.search_sparse([1], [1.0], [0, 1], 1025))
    refused(pkg, E_UNSUPPORTED, lambda: ix.search_bm25([[1]], 1025))
    assert state(ix) == before
    assert same(ix.search_sparse(*flat(qs), 10), want[10])


def test_three_adds_equal_one_add(base, pkg):
    ix, corpus, qs, want = base
    docs = corpus.docs
    with pkg.Mi355Index(8, "cosine", device=0) as three:
        three.set_option("sparse_tile_docs", TILE)
        three.add_sparse(docs[:300])
        mid = sparse_ref.SparseCorpus(docs[:300])
        assert same(three.search_sparse(*flat(qs), 10), sparse_ref.search_weighted(mid, qs, 10))   # the layout is rebuilt after an add
        terms = [t for d in docs[300:301] for t in d]
        three.add_sparse(terms, [0, len(terms)])                                                 # the (terms, offsets) form
        three.add_sparse(docs[301:])
        assert state(three) == state(ix)
        assert same(three.search_sparse(*flat(qs), 1024), want[1024])


def test_bm25_layer_df_and_stats(base):
    ix, corpus, qs, _ = base
    probe = [0, 1, 17, RARE, VOCAB + 100, (1 << 20) - 1, 1 << 20, -5]
    assert ix.sparse_df(probe).tolist() == [corpus.df(t) for t in probe]
    assert ix.sparse_df([0])[0] == N_BASE - 3
    assert state(ix) == [N_BASE, corpus.n_live, corpus.total_len, corpus.n_postings, corpus.vocab]
    rng = np.random.default_rng(13)
    raw = [rng.choice(VOCAB + 50, size=int(rng.integers(1, 25))).tolist() for _ in range(20)] + [[], list(UNSEEN), [RARE, RARE, 1 << 20, -3]]
    want = sparse_ref.search_bm25(corpus, raw, 10)
    ix.reset_stats()
    got = ix.search_bm25(raw, 10)
    assert same(got, want)
    assert (ix.stat("sparse_searches"), ix.stat("sparse_queries")) == (1, len(raw))
    assert ix.stat("sparse_postings_scored") == sum(corpus.df(t) for q in raw for t in set(q) if 0 <= t < (1 << 20))
    # the same through the weighted layer, with the weights math.log gives
    weighted = [sparse_ref.bm25_weights(corpus, q) for q in raw]
    N = corpus.n_live
    assert weighted[0][1] == [math.log(1.0 + ((N - corpus.df(t)) + 0.5) / (corpus.df(t) + 0.5)) for t in weighted[0][0]]
    assert same(ix.search_sparse(*flat(weighted), 10), want)
    assert ix.stat("sparse_overflows") == 0


def test_tiny_candidate_lists_overflow_and_redo(base, pkg):
    ix, corpus, qs, want = base
    with pkg.Mi355Index(8, "cosine", device=0) as tiny:
        tiny.set_option("sparse_tile_docs", TILE)
        tiny.set_option("sparse_cand_cap", 16)
        tiny.add_sparse(corpus.docs)
        # at k = 1024 the kept list never fills, so every match is a candidate: the launch over documents [32, 64) alone
        # brings query 0 (term 0: every document) 32 of them
        assert same(tiny.search_sparse(*flat(qs), 10), want[10])
        assert same(tiny.search_sparse(*flat(qs), 1024), want[1024])
        assert tiny.stat("sparse_overflows") > 0


def test_default_options_several_launches(pkg):
    """5000 documents under the default tile (2048) and candidate list (2048): three tiles, and two (k = 10) or three
    (k = 1024) launches whose later ones append only what beats the k-th kept entry of the earlier ones"""
    rng = np.random.default_rng(41)
    docs = zipf_docs(rng, 5000, 300, max_len=30)
    qs = [(rng.choice(300, size=int(rng.integers(1, 12)), replace=False).tolist(), None) for _ in range(11)] + [([0], None)]
    qs = [(t, rng.uniform(0.2, 3.0, size=len(t)).tolist()) for t, _ in qs]
    corpus = sparse_ref.SparseCorpus(docs)
    with pkg.Mi355Index(8, "cosine", device=0) as ix:
        ix.add_sparse(docs)
        for k in (10, 1024):
            assert same(ix.search_sparse(*flat(qs), k), sparse_ref.search_weighted(corpus, qs, k))
        assert ix.stat("sparse_postings_scored") == 2 * sum(corpus.df(t) for q in qs for t in q[0]) or ix.stat("sparse_overflows") > 0


def test_device_forms_equal_host_forms(base):
    ix, corpus, qs, want = base
    assert same(ix.search_sparse(*flat(qs), 10, device_out=True), want[10])
    raw = [q[0] + q[0] for q in qs]
    assert same(ix.search_bm25(raw, 10, device_out=True), ix.search_bm25(raw, 10))
    assert same(ix.search_bm25(raw, 10, device_out=True), sparse_ref.search_bm25(corpus, raw, 10))


def test_row_offset_empty_store_and_views(pkg):
    rng = np.random.default_rng(21)
    docs = zipf_docs(rng, 300, 50, max_len=20)
    corpus = sparse_ref.SparseCorpus(docs)
    qs = [([1, 2, 3], [1.0, 2.0, 0.5]), ([0], [1.0])]
    with pkg.Mi355Index(8, "cosine", device=0) as ix:
        d, r = ix.search_sparse(*flat(qs), 4)                     # an empty store
        assert (r == -1).all() and np.isnan(d).all() and ix.size_sparse() == 0
        ix.add_sparse([[], []])                                   # documents without tokens only: still nothing to match
        d, r = ix.search_bm25([[1]], 4)
        assert (r == -1).all() and np.isnan(d).all() and ix.size_sparse() == 2 and ix.stat("sparse_docs") == 0
    with pkg.Mi355Index(8, "cosine", device=0) as ix:
        ix.set_option("sparse_tile_docs", TILE)
        ix.set_option("row_offset", 5_000_000_000)
        ix.add_sparse(docs)
        assert same(ix.search_sparse(*flat(qs), 6), sparse_ref.search_weighted(corpus, qs, 6, row_offset=5_000_000_000))
        ix.set_option("row_offset", 0)
        resident = ix.stat("hbm_bytes_resident")
        assert resident >= corpus.n_postings * 6 + 300 * 12
        # a view has an empty sparse store and refuses the add
        ix.add(rng.standard_normal((40, 8)).astype(np.float32))
        with ix.view(row_ids=np.arange(10)) as v:
            assert v.size_sparse() == 0
            refused(pkg, E_INVALID, lambda: v.add_sparse([[1]]))
            d, r = v.search_bm25([[1]], 3)
            assert (r == -1).all() and np.isnan(d).all()


def test_dense_search_on_the_same_handle_is_untouched(pkg, oracle):
    rng = np.random.default_rng(31)
    C = rng.standard_normal((3000, 64)).astype(np.float32)
    Q = rng.standard_normal((9, 64)).astype(np.float32)
    docs = zipf_docs(rng, 400, 80, max_len=30)
    corpus = sparse_ref.SparseCorpus(docs)
    qs = [([0, 3, 7], [1.0, 1.0, 2.0])]
    with pkg.Mi355Index(64, "cosine", device=0) as ix:
        ix.add(C)
        d0, r0 = ix.search(Q, 10)
        ix.set_option("sparse_tile_docs", TILE)
        ix.add_sparse(docs)
        got = ix.search_sparse(*flat(qs), 10)
        d1, r1 = ix.search(Q, 10)
        assert same(got, sparse_ref.search_weighted(corpus, qs, 10))
        assert np.array_equal(r0, r1) and np.array_equal(d0.view(np.uint64), d1.view(np.uint64))
        rd, rr = oracle.topk_search(C, Q, 10)
        assert np.array_equal(r1, rr) and np.array_equal(d1, rd)
        ix.compact()                                              # does not touch the sparse store
        assert same(ix.search_sparse(*flat(qs), 10), got)
