"""CPU reference of the row-sharded sparse searches (include/mi355dr.h "row-sharded sparse search"), built on tests/sparse_ref.py.

The shards are sparse_ref.SparseCorpus objects holding consecutive runs of the documents.  What the library gathers is summed
here: N (documents with tokens), total_len and the df of the query's terms -- integers, so the sums are exact.  Every shard is
then scored by sparse_ref.search_weighted's own operations with the GLOBAL avgdl in the norms and the GLOBAL N and df in the
BM25 weights, returning global ids, and the per-shard lists are merged under (distance asc, NaN last, id asc).  The score forms
fold per position: the value of the lowest shard whose value is not NaN (at most one shard owns a document).

`own_statistics=True` scores every shard with ITS OWN N, total_len and df instead: what a naive sharding computes, and what the
tests must be able to tell from the above.
"""

import copy
import math

import numpy as np

import sparse_ref
import sparse_subset_ref


def shard_offsets(shards):
    """global id of each shard's first document"""
    return np.concatenate([[0], np.cumsum([len(s) for s in shards])]).astype(np.int64)[:-1].tolist()


def global_stats(shards):
    return sum(s.n_live for s in shards), sum(s.total_len for s in shards)


def global_df(shards, t):
    return sum(s.df(t) for s in shards)


def with_global_stats(shard, n_live, total_len):
    """the shard as sparse_ref scores it, under the statistics of all shards"""
    view = copy.copy(shard)
    view.n_live, view.total_len = n_live, total_len
    return view


def bm25_weights(shards, tokens):
    """raw query tokens -> (terms ascending, each once, GLOBAL df > 0; idf weights by math.log from the global N and df)"""
    N, _ = global_stats(shards)
    terms = [t for t in sorted(set(int(t) for t in tokens)) if 0 <= t < sparse_ref.TERM_LIMIT and global_df(shards, t) > 0]
    return terms, [math.log(1.0 + ((float(N - global_df(shards, t)) + 0.5) / (float(global_df(shards, t)) + 0.5))) for t in terms]


def merge_lists(dists, rows, k):
    """per-shard lists [world][B, k] -> [B, k] under (distance asc, NaN last, id asc); NaN / -1 behind"""
    B = dists[0].shape[0]
    out_d = np.full((B, k), np.nan, dtype=np.float64)
    out_r = np.full((B, k), -1, dtype=np.int64)
    d_all, r_all = np.concatenate(dists, axis=1), np.concatenate(rows, axis=1)
    for j in range(B):
        keep = r_all[j] >= 0
        d, r = d_all[j][keep], r_all[j][keep]
        nan = np.isnan(d)
        bits = np.where(nan, 0.0, d).view(np.int64)
        key = bits ^ ((bits >> 63) & np.int64(0x7FFFFFFFFFFFFFFF))  # (value asc, -0.0 before +0.0)
        order = np.lexsort((r, key, nan))[:k]
        out_d[j, :order.size], out_r[j, :order.size] = d[order], r[order]
    return out_d, out_r


def _per_shard(shards, own_statistics):
    N, total = global_stats(shards)
    for shard, off in zip(shards, shard_offsets(shards)):
        yield (shard if own_statistics else with_global_stats(shard, N, total)), off


def search_weighted(shards, queries, k, k1=1.2, b=0.75, doc_ids=None, own_statistics=False):
    """queries: (terms, weights) pairs.  doc_ids: None, or the listed GLOBAL ids the search is restricted to."""
    dists, rows = [], []
    for view, off in _per_shard(shards, own_statistics):
        if view.n_live == 0 or len(view) == 0:
            d, r = np.full((len(queries), k), np.nan), np.full((len(queries), k), -1, dtype=np.int64)
        elif doc_ids is None:
            d, r = sparse_ref.search_weighted(view, queries, k, k1, b, row_offset=off)
        else:
            d, r = sparse_subset_ref.search_weighted_subset(view, queries, k, doc_ids, k1, b, row_offset=off)
        dists.append(d)
        rows.append(r)
    return merge_lists(dists, rows, k)


def search_bm25(shards, token_lists, k, k1=1.2, b=0.75, doc_ids=None, own_statistics=False):
    if not own_statistics:
        return search_weighted(shards, [bm25_weights(shards, q) for q in token_lists], k, k1, b, doc_ids)
    dists, rows = [], []  # every shard under its own N, total_len and df: NOT the contract
    for shard, off in zip(shards, shard_offsets(shards)):
        if doc_ids is None:
            d, r = sparse_ref.search_bm25(shard, token_lists, k, k1, b, row_offset=off)
        else:
            d, r = sparse_subset_ref.search_bm25_subset(shard, token_lists, k, doc_ids, k1, b, row_offset=off)
        dists.append(d)
        rows.append(r)
    return merge_lists(dists, rows, k)


def fold_scores(per_shard):
    """[world][B, m] -> [B, m]: per position the value of the lowest shard whose value is not NaN"""
    out = per_shard[0].copy()
    for other in per_shard[1:]:
        out = np.where(np.isnan(out), other, out)
    return out


def score_weighted(shards, queries, doc_ids, k1=1.2, b=0.75):
    ids = np.asarray(doc_ids, dtype=np.int64).reshape(len(queries), -1)
    per = []
    for view, off in _per_shard(shards, False):
        if view.n_live == 0 or len(view) == 0:
            per.append(np.full(ids.shape, np.nan))
        else:
            per.append(sparse_subset_ref.score_weighted_subset(view, queries, ids, k1, b, row_offset=off))
    return fold_scores(per)


def score_bm25(shards, token_lists, doc_ids, k1=1.2, b=0.75):
    return score_weighted(shards, [bm25_weights(shards, q) for q in token_lists], doc_ids, k1, b)
