"""CPU: the reference of the row-sharded sparse searches (tests/sparse_shard_ref.py) against the one-corpus references.

Shards scored with the SUMMED statistics and merged under (distance asc, id asc) must be the whole corpus's answer bit for
bit; shards scored with their own statistics must not be, on this fixture -- else the GPU tests could not tell the two apart.
"""

import numpy as np
import pytest

import sparse_ref
import sparse_shard_ref
import sparse_subset_ref

N_DOCS, VOCAB = 420, 60
CUTS = {
    2: [150, 270],
    3: [200, 0, 220],                         # (an empty shard in the middle)
    8: [10, 90, 0, 55, 120, 1, 100, 44],      # (an empty one, and one of a single document)
}


def _corpus_docs():
    rng = np.random.default_rng(314)
    docs = []
    for i in range(N_DOCS):
        # short documents in front, long ones behind: a shard's avgdl is not the corpus's
        hi = 8 if i < N_DOCS // 2 else 30
        n = 0 if i % 17 == 3 else int(rng.integers(1, hi + 1))
        # the second half draws from the upper vocabulary more often: a shard's df is not a share of the corpus's
        lo_v = 0 if i < N_DOCS // 2 else VOCAB // 3
        docs.append(rng.integers(lo_v, VOCAB, size=n).tolist())
    docs[7] = [5, 5, 9]
    docs[N_DOCS - 4] = [5, 5, 9]  # two identical documents, far apart: one per shard in every cut
    return docs


@pytest.fixture(scope="module")
def docs():
    return _corpus_docs()


@pytest.fixture(scope="module")
def whole(docs):
    return sparse_ref.SparseCorpus(docs)


def _shards(docs, world):
    sizes = CUTS[world]
    assert sum(sizes) == len(docs)
    out, at = [], 0
    for n in sizes:
        out.append(sparse_ref.SparseCorpus(docs[at:at + n]))
        at += n
    return out


def _token_queries():
    rng = np.random.default_rng(2718)
    qs = [rng.integers(0, VOCAB + 5, size=int(rng.integers(1, 7))).tolist() for _ in range(14)]
    return qs + [[], [5, 9, 5], [VOCAB + 3], [-4, 1 << 21, 12]]  # no term; the twin documents; an unseen term; out of range


def _weighted_queries():
    rng = np.random.default_rng(1618)
    out = []
    for _ in range(10):
        terms = rng.choice(VOCAB + 3, size=int(rng.integers(1, 6)), replace=False).tolist()
        out.append((terms, rng.uniform(-1.0, 2.0, size=len(terms)).tolist()))
    return out + [([], [])]


def _same(a, b):
    return np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("world", sorted(CUTS))
@pytest.mark.parametrize("k", [1, 10, 100])
def test_global_statistics_give_the_whole_corpus_answer(docs, whole, world, k):
    shards = _shards(docs, world)
    assert sparse_shard_ref.global_stats(shards) == (whole.n_live, whole.total_len)
    assert any(len(s) == 0 for s in shards) == (world != 2)
    tq, wq = _token_queries(), _weighted_queries()
    assert _same(sparse_shard_ref.search_bm25(shards, tq, k), sparse_ref.search_bm25(whole, tq, k))
    assert _same(sparse_shard_ref.search_weighted(shards, wq, k, 0.9, 0.4), sparse_ref.search_weighted(whole, wq, k, 0.9, 0.4))


@pytest.mark.parametrize("world", sorted(CUTS))
def test_own_statistics_do_not(docs, whole, world):
    shards = _shards(docs, world)
    tq, wq = _token_queries(), _weighted_queries()
    assert not _same(sparse_shard_ref.search_bm25(shards, tq, 10, own_statistics=True), sparse_ref.search_bm25(whole, tq, 10))
    # the weighted form brings its own weights: the norms (avgdl) alone must already differ
    assert not _same(sparse_shard_ref.search_weighted(shards, wq, 10, own_statistics=True), sparse_ref.search_weighted(whole, wq, 10))


def test_twin_documents_come_in_id_order(docs, whole):
    d, r = sparse_shard_ref.search_bm25(_shards(docs, 2), [[5, 9, 5]], 100)
    at = {int(x): i for i, x in enumerate(r[0]) if x >= 0}
    assert at[N_DOCS - 4] == at[7] + 1 and d[0, at[7]] == d[0, at[N_DOCS - 4]]


@pytest.mark.parametrize("world", sorted(CUTS))
def test_subset_search_and_owner_wins_fold(docs, whole, world):
    shards = _shards(docs, world)
    tq, wq = _token_queries(), _weighted_queries()
    rng = np.random.default_rng(99)
    listed = np.concatenate([rng.integers(0, N_DOCS, size=130), [-1, N_DOCS, N_DOCS + 7, 7, 7, N_DOCS - 4]])
    assert _same(sparse_shard_ref.search_bm25(shards, tq, 10, doc_ids=listed), sparse_subset_ref.search_bm25_subset(whole, tq, 10, listed))
    assert _same(sparse_shard_ref.search_weighted(shards, wq, 10, doc_ids=listed),
                 sparse_subset_ref.search_weighted_subset(whole, wq, 10, listed))
    pool = rng.integers(-2, N_DOCS + 3, size=(len(tq), 12))
    pool[:, 3] = pool[:, 2]   # a duplicate in every row
    pool[:, 5] = -1
    pool[-3, :4] = [7, N_DOCS - 4, 7, 0]
    got, want = sparse_shard_ref.score_bm25(shards, tq, pool), sparse_subset_ref.score_bm25_subset(whole, tq, pool)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    assert (~np.isnan(want)).sum() > 20
    pw = pool[:len(wq)]
    got, want = sparse_shard_ref.score_weighted(shards, wq, pw), sparse_subset_ref.score_weighted_subset(whole, wq, pw)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


def test_no_document_anywhere():
    shards = [sparse_ref.SparseCorpus([[], []]), sparse_ref.SparseCorpus()]
    d, r = sparse_shard_ref.search_bm25(shards, [[1, 2]], 5)
    assert np.isnan(d).all() and (r == -1).all()
    assert np.isnan(sparse_shard_ref.score_bm25(shards, [[1, 2]], [[0, 1, 2]])).all()
