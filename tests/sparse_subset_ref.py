"""CPU reference of the sparse searches within a listed subset (include/mi355dr.h "sparse store", "Within a listed subset"),
built on tests/sparse_ref.py.

A filter, not a view: the statistics are the whole corpus's.  A result line is the unrestricted ranking -- sparse_ref's search
with k = len(corpus), every match under (distance asc, NaN last, id asc) -- with the unlisted documents struck out, cut to k,
NaN / -1 behind.  The score form is the same ranking read per document.  doc_ids are GLOBAL ids (local id + row_offset); ids
outside the corpus are skipped, duplicates count once in a search and once per position in a score block.
"""

import numpy as np

import sparse_ref


def local_ids(corpus, doc_ids, row_offset=0):
    """the listed local documents, ascending, each once"""
    n = len(corpus)
    return sorted({int(g) - row_offset for g in np.asarray(doc_ids, dtype=np.int64).reshape(-1).tolist() if 0 <= int(g) - row_offset < n})


def search_weighted_subset(corpus, queries, k, doc_ids, k1=1.2, b=0.75, row_offset=0):
    B = len(queries)
    dist = np.full((B, k), np.nan, dtype=np.float64)
    rows = np.full((B, k), -1, dtype=np.int64)
    listed = np.asarray(local_ids(corpus, doc_ids, row_offset), dtype=np.int64)
    if len(corpus) == 0 or listed.size == 0:
        return dist, rows
    full_d, full_r = sparse_ref.search_weighted(corpus, queries, len(corpus), k1, b)
    for j in range(B):
        keep = np.flatnonzero((full_r[j] >= 0) & np.isin(full_r[j], listed))[:k]
        dist[j, :keep.size] = full_d[j, keep]
        rows[j, :keep.size] = full_r[j, keep] + row_offset
    return dist, rows


def search_bm25_subset(corpus, token_lists, k, doc_ids, k1=1.2, b=0.75, row_offset=0):
    """the weights come from the WHOLE corpus's N and df"""
    return search_weighted_subset(corpus, [sparse_ref.bm25_weights(corpus, q) for q in token_lists], k, doc_ids, k1, b, row_offset)


def score_weighted_subset(corpus, queries, doc_ids, k1=1.2, b=0.75, row_offset=0):
    """doc_ids [B, m] -> distances [B, m]: NaN where the id is skipped or the document does not match"""
    ids = np.asarray(doc_ids, dtype=np.int64)
    ids = ids.reshape(len(queries), -1)
    out = np.full(ids.shape, np.nan, dtype=np.float64)
    if len(corpus) == 0 or ids.size == 0:
        return out
    full_d, full_r = sparse_ref.search_weighted(corpus, queries, len(corpus), k1, b)
    for q in range(len(queries)):
        of = {int(r): d for d, r in zip(full_d[q].tolist(), full_r[q].tolist()) if r >= 0}
        for j, g in enumerate(ids[q].tolist()):
            if g - row_offset in of:
                out[q, j] = of[g - row_offset]
    return out


def score_bm25_subset(corpus, token_lists, doc_ids, k1=1.2, b=0.75, row_offset=0):
    return score_weighted_subset(corpus, [sparse_ref.bm25_weights(corpus, q) for q in token_lists], doc_ids, k1, b, row_offset)


def postings_scored(corpus, queries, doc_ids, row_offset=0):
    """(query term, listed document) postings: what "sparse_postings_scored" grows by in a subset search"""
    listed = np.asarray(local_ids(corpus, doc_ids, row_offset), dtype=np.int64)
    return sum(int(np.isin(corpus.post[int(t)][0], listed).sum()) for terms, _ in queries for t in set(terms) if int(t) in corpus.post)


def sparse_subset_methods(cls):
    """Class decorator on top of sparse_ref.sparse_methods: the four *_subset methods of Mi355Index, answered by this reference."""
    cls = sparse_ref.sparse_methods(cls)

    def _c(self):
        if getattr(self, "_sparse", None) is None:
            self._sparse = sparse_ref.SparseCorpus()
        return self._sparse

    def _queries(terms, weights, offsets):
        return [(list(terms[offsets[i]:offsets[i + 1]]), list(weights[offsets[i]:offsets[i + 1]])) for i in range(len(offsets) - 1)]

    def search_sparse_subset(self, terms, weights, offsets, k, doc_ids, k1=1.2, b=0.75, device_out=False):
        return search_weighted_subset(_c(self), _queries(terms, weights, offsets), k, doc_ids, k1, b, getattr(self, "row_offset", 0))

    def search_bm25_subset(self, token_lists, k, doc_ids, k1=1.2, b=0.75, device_out=False, offsets=None):
        return globals()["search_bm25_subset"](_c(self), token_lists, k, doc_ids, k1, b, getattr(self, "row_offset", 0))

    def score_sparse_subset(self, terms, weights, offsets, doc_ids, k1=1.2, b=0.75):
        return score_weighted_subset(_c(self), _queries(terms, weights, offsets), doc_ids, k1, b, getattr(self, "row_offset", 0))

    def score_bm25_subset(self, token_lists, doc_ids, k1=1.2, b=0.75, offsets=None):
        return globals()["score_bm25_subset"](_c(self), token_lists, doc_ids, k1, b, getattr(self, "row_offset", 0))

    for f in (search_sparse_subset, search_bm25_subset, score_sparse_subset, score_bm25_subset):
        setattr(cls, f.__name__, f)
    return cls
