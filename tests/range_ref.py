"""CPU reference of the range search (include/mi355dr.h "range search"), restated in numpy for the tests.

It works from all-pairs float8 distances -- the oracle's, never the library's:
    in range = the row is live, its distance d is not NaN and d <= radius (compared as doubles);
    count    = the number of such rows;
    list     = their first max_results under (distance asc, row asc), NaN / -1 behind them.
"""

import numpy as np


def sort_pairs(D):
    """[B, n] distances by row -> (distances, rows) [B, n] in the library's total order: distance asc, NaN last, row asc.
    (A stable sort: numpy puts NaN last and equal values stay in row order.)"""
    D = np.asarray(D, dtype=np.float64)
    order = np.argsort(D, axis=1, kind="stable")
    return np.take_along_axis(D, order, axis=1), order.astype(np.int64)


def oracle_sorted(oracle, C, Q, metric="cosine", depth=None):
    """every pair's distance in the total order, by the oracle: its exact top-k at k = n (read-only arrays).  depth: only the
    nearest `depth` pairs per query -- enough for radii below each query's depth-th distance (`covers` checks that)."""
    k = len(C) if depth is None else min(depth, len(C))
    ds, rs = oracle.topk_search(C, Q, max(k, 1), metric=metric)
    ds, rs = ds[:, :k], rs[:, :k]
    ds.setflags(write=False)
    rs.setflags(write=False)
    return ds, rs


def covers(ds, radius):
    """a truncated oracle_sorted holds every in-range pair: each radius lies strictly below the query's last listed distance
    (a NaN there: every distance the query has is listed)"""
    with np.errstate(invalid="ignore"):
        return bool((np.isnan(ds[:, -1]) | (radius_array(radius, ds.shape[0]) < ds[:, -1])).all())


def radius_array(radius, B):
    r = np.asarray(radius, dtype=np.float64)
    return np.full(B, float(r)) if r.ndim == 0 else r


def search_range(ds, rs, radius, max_results, live=None):
    """(ds, rs): sort_pairs / oracle_sorted.  live: bool [n] (None: every row).  -> (dist [B, m], rows [B, m], count [B])"""
    B, m = ds.shape[0], int(max_results)
    radius = radius_array(radius, B)
    dist = np.full((B, m), np.nan, dtype=np.float64)
    rows = np.full((B, m), -1, dtype=np.int64)
    count = np.zeros(B, dtype=np.int64)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            keep = ~np.isnan(ds[b]) & (ds[b] <= radius[b]) & (rs[b] >= 0)
        if live is not None:
            keep &= np.asarray(live, dtype=bool)[np.maximum(rs[b], 0)]
        at = np.flatnonzero(keep)
        count[b] = len(at)
        at = at[:m]
        dist[b, :len(at)] = ds[b, at]
        rows[b, :len(at)] = rs[b, at]
    return dist, rows, count


def radius_admitting(ds, rs, want, live=None):
    """per query the radius that admits exactly the `want[b]` nearest live rows with a distance: the want-th of them (its own
    bits: that row is included); -inf for 0.  Returns (radius [B], the counts a reference pass confirms)."""
    B = ds.shape[0]
    want = np.broadcast_to(np.asarray(want, dtype=np.int64), (B,))
    radius = np.full(B, -np.inf, dtype=np.float64)
    for b in range(B):
        ok = ~np.isnan(ds[b]) & (rs[b] >= 0)
        if live is not None:
            ok &= np.asarray(live, dtype=bool)[np.maximum(rs[b], 0)]
        vals = ds[b, ok]
        if want[b] > 0 and len(vals) > 0:
            radius[b] = vals[min(want[b], len(vals)) - 1]
    return radius, search_range(ds, rs, radius, 1, live)[2]


def same(got, exp):
    """all distances bit for bit (NaN where NaN), all rows, all counts"""
    (gd, gr, gc), (ed, er, ec) = got, exp
    assert gd.shape == ed.shape and gr.shape == er.shape and gc.shape == ec.shape
    assert np.array_equal(gc, ec), f"counts differ at {np.flatnonzero(gc != ec)[:8]}: {gc[gc != ec][:8]} vs {ec[gc != ec][:8]}"
    assert np.array_equal(gr, er), f"rows differ in queries {np.flatnonzero((gr != er).any(axis=1))[:8]}"
    nan = np.isnan(ed)
    assert np.array_equal(np.isnan(gd), nan)
    assert np.array_equal(gd[~nan].view(np.uint64), ed[~nan].view(np.uint64))
