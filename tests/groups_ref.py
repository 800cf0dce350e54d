"""CPU reference of the grouped merge (include/mi355dr.h "grouped search"), restated in numpy for the tests.

Every (value, row) entry of a group's lists with row >= 0 takes part; the order key of a value is computed from the double's
bits as the library's dist_to_key does (a negative number's bits inverted, the sign bit set on the others, every NaN the
largest key), so -0.0 orders before +0.0 and a NaN behind every number.  A row is kept once, at its smallest key; the result
is sorted by (key, row) and cut at k; the tail is NaN / -1; count is the number of distinct rows.
"""

import numpy as np

KEY_NAN = np.uint64(0xFFFFFFFFFFFFFFFF)


def dist_to_key(vals) -> np.ndarray:
    v = np.ascontiguousarray(vals, dtype=np.float64)
    b = v.view(np.uint64)
    key = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(0x8000000000000000))
    return np.where(np.isnan(v), KEY_NAN, key)


def merge_groups(vals, rows, group_offsets, k):
    """vals float64 [S, width], rows int64 [S, width], group_offsets [G + 1] -> (vals [G,k], rows [G,k], count int32 [G])"""
    vals = np.ascontiguousarray(vals, dtype=np.float64)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    offs = np.asarray(group_offsets, dtype=np.int64)
    G = offs.shape[0] - 1
    out_v = np.full((G, k), np.nan)
    out_r = np.full((G, k), -1, dtype=np.int64)
    count = np.zeros(G, dtype=np.int32)
    for g in range(G):
        v = vals[offs[g]:offs[g + 1]].reshape(-1)
        r = rows[offs[g]:offs[g + 1]].reshape(-1)
        has = r >= 0
        v, r = v[has], r[has]
        if r.size == 0:
            continue
        key = dist_to_key(v)
        by_row = np.lexsort((key, r))
        first = np.ones(r.size, dtype=bool)
        first[1:] = r[by_row][1:] != r[by_row][:-1]
        keep = by_row[first]  # every row's occurrence with the smallest key
        count[g] = keep.size
        order = keep[np.lexsort((r[keep], key[keep]))][:k]
        out_v[g, :order.size] = np.where(np.isnan(v[order]), np.nan, v[order])
        out_r[g, :order.size] = r[order]
    return out_v, out_r, count


def same(a, b):
    """two (vals, rows[, count]) results agree bit for bit (NaN positions, not payloads)"""
    (va, ra), (vb, rb) = a[:2], b[:2]
    assert va.shape == vb.shape and ra.shape == rb.shape
    assert np.array_equal(ra, rb)
    assert np.array_equal(np.isnan(va), np.isnan(vb))
    ok = ~np.isnan(va)
    assert np.array_equal(np.ascontiguousarray(va[ok]).view(np.uint64), np.ascontiguousarray(vb[ok]).view(np.uint64))
    if len(a) > 2 and len(b) > 2 and a[2] is not None and b[2] is not None:
        assert np.array_equal(np.asarray(a[2], dtype=np.int64), np.asarray(b[2], dtype=np.int64))
