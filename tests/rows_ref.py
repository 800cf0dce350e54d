"""CPU reference of the search by stored row (include/mi355dr.h "search by stored row"), restated in numpy for the tests.

It works from the oracle's distances, never the library's:
    the query of slot b = the stored vector of row row_ids[b] (global id = local row + row_offset);
    a slot whose id is outside the index, or names a removed row, gives a NaN / -1 line and count 0;
    top-k form   = the first k of the live rows OTHER than the row itself (include_self: of all live rows) under the library's
                   total order (distance asc, NaN last, row asc), NaN / -1 behind them;
    range form   = tests/range_ref.py over the same distances with the row itself masked out before counting.
"""

import numpy as np

import range_ref


def _slots(C, row_ids, live, row_offset):
    """(local rows int64 [B], valid bool [B])"""
    ids = np.asarray(row_ids, dtype=np.int64).reshape(-1)
    local = ids - int(row_offset)
    valid = (local >= 0) & (local < len(C))
    if live is not None:
        valid &= np.asarray(live, dtype=bool)[np.where(valid, local, 0)]
    return local, valid


def search_rows(oracle, C, row_ids, k, metric="cosine", live=None, include_self=False, row_offset=0):
    """-> (dist float64 [B, k], rows int64 [B, k], global).  The oracle's total order of every valid slot's vector against C,
    as deep as the answer can reach: among the first k + 1 + (removed rows) entries at most one is the row itself and at most
    (removed rows) are dead, so k of the wanted rows are there -- or the order has ended."""
    C = np.ascontiguousarray(C, dtype=np.float32)
    n, k = len(C), int(k)
    local, valid = _slots(C, row_ids, live, row_offset)
    dist = np.full((len(local), k), np.nan, dtype=np.float64)
    rows = np.full((len(local), k), -1, dtype=np.int64)
    at = np.flatnonzero(valid)
    if len(at) == 0 or n == 0:
        return dist, rows
    n_dead = 0 if live is None else int((~np.asarray(live, dtype=bool)).sum())
    depth = min(n, k + 1 + n_dead)
    ds, rs = oracle.topk_search(C, np.ascontiguousarray(C[local[at]]), depth, metric=metric)
    for i, b in enumerate(at):
        keep = rs[i] >= 0
        if live is not None:
            keep &= np.asarray(live, dtype=bool)[np.maximum(rs[i], 0)]
        if not include_self:
            keep &= rs[i] != local[b]
        pos = np.flatnonzero(keep)[:k]
        dist[b, :len(pos)] = ds[i, pos]
        rows[b, :len(pos)] = rs[i, pos] + int(row_offset)
    return dist, rows


def self_masked_sorted(oracle, C, local_rows, metric="cosine", include_self=False):
    """(ds, rs) of range_ref.oracle_sorted for the stored vectors of `local_rows` (all valid), the entry of the row itself
    turned into "no entry" (row -1: range_ref never counts or lists it)"""
    local_rows = np.asarray(local_rows, dtype=np.int64)
    ds, rs = range_ref.oracle_sorted(oracle, C, np.ascontiguousarray(C[local_rows]), metric)
    if not include_self:
        rs = np.where(rs == local_rows[:, None], -1, rs)
        rs.setflags(write=False)
    return ds, rs


def search_range_rows(oracle, C, row_ids, radius, max_results, metric="cosine", live=None, include_self=False, row_offset=0):
    """-> (dist [B, m], rows [B, m] global, count [B])"""
    C = np.ascontiguousarray(C, dtype=np.float32)
    m = int(max_results)
    local, valid = _slots(C, row_ids, live, row_offset)
    B = len(local)
    radius = range_ref.radius_array(radius, B)
    dist = np.full((B, m), np.nan, dtype=np.float64)
    rows = np.full((B, m), -1, dtype=np.int64)
    count = np.zeros(B, dtype=np.int64)
    at = np.flatnonzero(valid)
    if len(at) == 0 or len(C) == 0:
        return dist, rows, count
    ds, rs = self_masked_sorted(oracle, C, local[at], metric, include_self)
    d, r, c = range_ref.search_range(ds, rs, radius[at], m, live)
    dist[at], rows[at], count[at] = d, np.where(r >= 0, r + int(row_offset), -1), c
    return dist, rows, count


def same(got, exp):
    """all distances bit for bit (NaN where NaN), all rows -- and all counts where both sides carry them"""
    assert len(got) == len(exp)
    if len(got) == 3:
        return range_ref.same(got, exp)
    (gd, gr), (ed, er) = got, exp
    assert gd.shape == ed.shape and gr.shape == er.shape
    assert np.array_equal(gr, er), f"rows differ in slots {np.flatnonzero((gr != er).any(axis=1))[:8]}"
    nan = np.isnan(ed)
    assert np.array_equal(np.isnan(gd), nan)
    assert np.array_equal(gd[~nan].view(np.uint64), ed[~nan].view(np.uint64))
