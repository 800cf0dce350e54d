"""GPU: the grouped merge (mi355dr_merge_groups_device) and the grouped search (mi355dr_search_groups / _device) against the
numpy restatement in tests/groups_ref.py, bit for bit: values, rows and counts.

The merge is checked at the smallest shapes at which k_merge_groups can go wrong (one list, ragged groups, a size that is no
power of two, the 4096-entry cap and one list beyond it, duplicates only, padding only, NaN beside a number, signed zeros,
rows above 2^33, k beyond the union, an empty group, no group, no counter); the search over `index.search(Q, fetch_k)`."""

import ctypes

import numpy as np
import pytest

import groups_ref
from groups_ref import same

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
N, D = 4096, 64


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


@pytest.fixture(scope="module")
def gauss(pkg):
    rng = np.random.default_rng(2024)
    C = rng.standard_normal((N, D)).astype(np.float32)
    with pkg.Mi355Index(D) as idx:
        idx.add(C)
        yield idx, C


def ragged_offsets(rng, S, lo=1, hi=5):
    sizes = []
    while sum(sizes) < S:
        sizes.append(min(int(rng.integers(lo, hi + 1)), S - sum(sizes)))
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def check_merge(idx, vals, rows, offs, k):
    """merge_groups == groups_ref, with and without the counter"""
    want = groups_ref.merge_groups(vals, rows, offs, k)
    same(idx.merge_groups(vals, rows, offs, k), want)
    got = idx.merge_groups(vals, rows, offs, k, want_count=False)
    assert got[2] is None
    same(got, want)
    return want


def random_lists(rng, S, width, n_rows):
    """S lists of `width` entries over few rows (many duplicates across and inside lists), some without a row"""
    vals = rng.standard_normal((S, width))
    rows = rng.integers(0, n_rows, (S, width)).astype(np.int64)
    rows[rng.random((S, width)) < 0.1] = -1
    return vals, rows


# ---- 1. the merge alone ----------------------------------------------------------------------------------------------------

def test_one_list_per_group_is_the_identity(gauss):
    idx, C = gauss
    dist, rows = idx.search(C[:3] + 0.1, 8)
    offs = np.arange(4, dtype=np.int32)
    want = check_merge(idx, dist, rows, offs, 8)
    same(want, (dist, rows))
    assert want[2].tolist() == [8, 8, 8]


@pytest.mark.parametrize("sizes,width", [((1, 2, 4, 3), 6), ((3,), 5), ((2, 1, 5), 33), ((4, 1), 1024)],
                         ids=["ragged", "n15-not-pow2", "n165", "n4096-cap"])
def test_ragged_groups_and_sizes(gauss, sizes, width):
    idx, _ = gauss
    rng = np.random.default_rng(width)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    vals, rows = random_lists(rng, int(offs[-1]), width, n_rows=max(8, width * 2))
    for k in (1, width, 2 * width):
        check_merge(idx, vals, rows, offs, k)


def test_beyond_the_cap_is_refused(gauss, pkg):
    idx, _ = gauss
    rng = np.random.default_rng(5)
    vals, rows = random_lists(rng, 6, 1024, 5000)
    before = idx.stat("groups_merged")
    with pytest.raises(pkg.NativeError) as e:
        idx.merge_groups(vals, rows, [0, 1, 6], 10)      # 5 x 1024 entries in one group
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(pkg.NativeError) as e:
        idx.merge_groups(vals, rows, [0, 3, 6], 4097)    # k_out above 4096
    assert e.value.code == E_UNSUPPORTED
    assert idx.stat("groups_merged") == before
    check_merge(idx, vals, rows, [0, 2, 6], 10)          # 4 x 1024: the cap itself, and the handle still works
    assert idx.stat("groups_merged") == before + 4       # (two calls of two groups)


def test_duplicates_padding_nan_zeros(gauss):
    idx, _ = gauss
    rng = np.random.default_rng(7)
    # every list identical: the union is one list
    one_v, one_r = np.sort(rng.standard_normal(9)), rng.permutation(40)[:9].astype(np.int64)
    want = check_merge(idx, np.tile(one_v, (4, 1)), np.tile(one_r, (4, 1)), [0, 4], 12)
    assert want[2].tolist() == [9] and np.array_equal(want[1][0, :9], one_r) and (want[1][0, 9:] == -1).all()
    # every row -1: nothing
    want = check_merge(idx, rng.standard_normal((3, 5)), np.full((3, 5), -1), [0, 1, 3], 4)
    assert want[2].tolist() == [0, 0] and (want[1] == -1).all() and np.isnan(want[0]).all()
    # NaN beside a number of the same row (the number stays), a row that is NaN everywhere (it stays, last), negative rows
    vals = np.array([[np.nan, 0.5, np.nan, 0.1], [0.25, np.nan, np.nan, np.nan]])
    rows = np.array([[3, 9, 5, -1], [3, 5, 9, -2]])
    want = check_merge(idx, vals, rows, [0, 2], 4)
    assert want[1].tolist() == [[3, 9, 5, -1]] and want[2].tolist() == [3]
    assert want[0][0, :2].tolist() == [0.25, 0.5] and np.isnan(want[0][0, 2:]).all()
    # signed zeros: -0.0 is the smaller value, and both keep their bits
    vals = np.array([[0.0, -0.0, 0.0], [-0.0, 0.0, 1.0]])
    rows = np.array([[1, 2, 3], [1, 4, 2]])
    want = check_merge(idx, vals, rows, [0, 2], 5)
    assert want[1].tolist() == [[1, 2, 3, 4, -1]]
    assert np.signbit(want[0][0, :4]).tolist() == [True, True, False, False]


def test_rows_above_2_pow_33(gauss):
    idx, _ = gauss
    rng = np.random.default_rng(11)
    vals, rows = random_lists(rng, 7, 9, 20)
    big = np.where(rows >= 0, rows * (1 << 31) + (1 << 33) + (rows % 3), -1)   # distinct high AND low words
    want = check_merge(idx, vals, big, [0, 3, 7], 12)
    assert want[1].max() > 1 << 33
    # two rows that differ only above bit 32 stay two rows
    want = check_merge(idx, np.array([[0.5, 0.25]]), np.array([[(1 << 33) + 7, (1 << 34) + 7]]), [0, 1], 3)
    assert want[2].tolist() == [2]


def test_k_beyond_the_union_empty_group_no_group(gauss):
    idx, _ = gauss
    rng = np.random.default_rng(13)
    vals, rows = random_lists(rng, 5, 4, 6)
    offs = [0, 2, 2, 5, 5]            # groups 1 and 3 are empty
    for k in (3, 7, 25, 100):          # below / above the distinct count (<= 6), above n = 12, above next_pow2(n)
        want = check_merge(idx, vals, rows, offs, k)
        assert want[2][1] == 0 and want[2][3] == 0 and (want[1][[1, 3]] == -1).all()
    v, r, c = idx.merge_groups(np.empty((0, 4)), np.empty((0, 4), dtype=np.int64), [0], 5)   # G = 0
    assert v.shape == (0, 5) and r.shape == (0, 5) and c.shape == (0,)
    want = check_merge(idx, np.empty((0, 4)), np.empty((0, 4), dtype=np.int64), [0, 0, 0], 5)  # S = 0, two empty groups
    assert want[2].tolist() == [0, 0]


def test_merge_refusals_leave_the_handle_usable(gauss, pkg):
    idx, _ = gauss
    vals, rows = np.zeros((4, 3)), np.arange(12, dtype=np.int64).reshape(4, 3)
    before = idx.stat("groups_merged")
    for offs in ([1, 4], [0, 3, 2, 4], [0, 3], [0, 5]):   # not starting at 0, decreasing, not ending at S (twice)
        with pytest.raises(pkg.NativeError) as e:
            idx.merge_groups(vals, rows, offs, 2)
        assert e.value.code == E_INVALID, offs
    with pytest.raises(pkg.NativeError) as e:
        idx.merge_groups(vals, rows, [0, 4], 0)
    assert e.value.code == E_INVALID
    lib, h, offs = idx._lib, idx._h, np.array([0, 4], dtype=np.int32)
    op = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    buf = idx.dev_alloc(4 * 3 * 8)
    try:
        raw = lambda **kw: lib.mi355dr_merge_groups_device(  # noqa: E731
            h, kw.get("vals", buf), kw.get("rows", buf), kw.get("S", 4), kw.get("width", 3), kw.get("offs", op), kw.get("G", 1),
            kw.get("k", 2), kw.get("out", buf), kw.get("out", buf), None, None)
        assert raw(G=-1) == E_INVALID
        assert raw(width=0) == E_INVALID
        assert raw(k=-3) == E_INVALID
        assert raw(offs=None) == E_INVALID
        assert raw(vals=None) == E_INVALID
        assert raw(out=None) == E_INVALID
        assert lib.mi355dr_merge_groups_device(h, None, None, 0, 3, None, 0, 2, None, None, None, None) == 0   # G = 0: a no-op
    finally:
        idx.dev_free(buf)
    assert idx.stat("groups_merged") == before
    check_merge(idx, vals, rows, [0, 4], 2)


# ---- 2. the grouped search -------------------------------------------------------------------------------------------------

def queries_near(rng, C, S, noise=0.3):
    """sub-queries in runs around the same rows: the lists of a group overlap"""
    base = C[rng.integers(0, C.shape[0], (S + 2) // 3).repeat(3)[:S]]
    return (base + noise * rng.standard_normal(base.shape)).astype(np.float32)


def check_search(idx, Q, offs, k, fetch_k):
    want = groups_ref.merge_groups(*idx.search(Q, fetch_k), offs, k)
    same(idx.search_groups(Q, offs, k, fetch_k), want)
    return want


@pytest.mark.parametrize("metric", ["cosine", "ip"])
@pytest.mark.parametrize("fetch_k", [1, 7, 64, 1024])
def test_search_groups_fetch_k_and_k(pkg, gauss, metric, fetch_k):
    _, C = gauss
    rng = np.random.default_rng(fetch_k)
    d = 64 if metric == "cosine" else 50
    Cm = np.ascontiguousarray(C[:2500, :d])
    S = 11
    Q = queries_near(rng, Cm, S)
    offs = ragged_offsets(rng, S, 1, 4)
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(Cm)
        for k in sorted({1, fetch_k, 2 * fetch_k}):
            want = check_search(idx, Q, offs, k, fetch_k)
            assert (want[2] >= fetch_k).all()
        if fetch_k == 7:   # fetch_k defaults to k; a single query without a batch axis
            same(idx.search_groups(Q, offs, 7), idx.search_groups(Q, offs, 7, 7))
            same(idx.search_groups(Q[0], [0, 1], 7), idx.search(Q[:1], 7))


def test_two_internal_blocks_with_a_group_across_them(gauss):
    idx, C = gauss
    rng = np.random.default_rng(1030)
    S = 1030
    offs = ragged_offsets(rng, S, 1, 5)
    inner = offs[(offs > 0) & (offs < S)]
    if 1024 in inner:   # make a group straddle the block boundary at query 1024
        offs = offs[offs != 1024]
    assert 1024 not in offs and offs[-1] == S
    Q = queries_near(rng, C, S)
    idx.reset_stats()
    want = check_search(idx, Q, offs, 10, 7)
    G = offs.shape[0] - 1
    assert (want[2] <= 70).all() and (want[2] >= 7).all()
    assert (idx.stat("group_searches"), idx.stat("group_subqueries"), idx.stat("groups_merged")) == (1, S, G)
    idx.merge_groups(want[0], want[1], [0, 2, G], 3)
    assert (idx.stat("group_searches"), idx.stat("group_subqueries"), idx.stat("groups_merged")) == (1, S, G + 2)


def test_removed_rows_and_row_offset(pkg):
    """fewer live rows than fetch_k (NaN / -1 tails inside the lists), a zero row (NaN with a row), global rows above 2^33"""
    rng = np.random.default_rng(23)
    C = rng.standard_normal((60, 50)).astype(np.float32)
    C[4] = 0.0
    off = (1 << 33) + 12345
    with pkg.Mi355Index(50) as idx:
        idx.set_option("row_offset", off)
        idx.add(C)
        idx.remove_rows(np.arange(20, 45))   # (the index's own row numbers; the results carry row_offset)
        Q = queries_near(rng, C, 7)
        offs = [0, 3, 4, 7]
        for k, fetch_k in ((10, 40), (40, 40), (80, 40), (5, 7)):
            want = check_search(idx, Q, offs, k, fetch_k)
            assert want[1].max() > 1 << 33 and (want[2] <= 35).all()
        assert (check_search(idx, Q, offs, 80, 40)[2] == 35).all()   # every live row, the zero row (NaN) included


def test_view_answers_under_the_parents_ids(pkg, gauss):
    idx, C = gauss
    rng = np.random.default_rng(29)
    ids = np.arange(3, N, 7)
    Q = queries_near(rng, C[ids], 9)
    offs = [0, 2, 5, 9]
    with idx.view(row_ids=ids) as v:
        want = check_search(v, Q, offs, 12, 9)
        assert np.isin(want[1], ids).all()
        same(want, groups_ref.merge_groups(*idx.search_subset(Q, 9, ids), offs, 12))
        check_merge(v, want[0], want[1], [0, 3], 5)   # the stateless merge is allowed on a view


def test_device_form_behind_an_async_block(gauss):
    idx, C = gauss
    rng = np.random.default_rng(31)
    S, k, fetch_k = 9, 12, 8
    Q = queries_near(rng, C, S)
    offs = np.array([0, 4, 4, 9], dtype=np.int32)
    G = 3
    want = groups_ref.merge_groups(*idx.search(Q, fetch_k), offs, k)
    plain = idx.search(Q, 5)
    ptrs = [idx.dev_alloc(n) for n in (Q.nbytes, G * k * 8, G * k * 8, G * 4, S * 5 * 8, S * 5 * 8)]
    pq, od, orr, oc, ad, ar = ptrs
    try:
        idx.dev_upload(pq, Q)
        for with_count in (True, False):
            idx.dev_upload(orr, np.full((G, k), -7, np.int64))
            idx.dev_upload(oc, np.full(G, -7, np.int32))
            ticket = idx.search_device_async(pq, S, 5, ad, ar)            # in flight: search_groups completes it first
            idx.search_groups_device(pq, offs, k, fetch_k, od, orr, oc if with_count else None)
            gd, gr, gc = np.empty((G, k)), np.empty((G, k), dtype=np.int64), np.empty(G, dtype=np.int32)
            for p, a in ((od, gd), (orr, gr), (oc, gc)):
                idx.dev_download(p, a)
            same((gd, gr, gc if with_count else None), want)
            if not with_count:
                assert (gc == -7).all()
            idx.search_wait(ticket)
            ga, gb = np.empty((S, 5)), np.empty((S, 5), dtype=np.int64)
            idx.dev_download(ad, ga)
            idx.dev_download(ar, gb)
            same((ga, gb), plain)
    finally:
        for p in ptrs:
            idx.dev_free(p)


def test_rows_are_the_top_k_of_the_groupwise_minimum(pkg, gauss, oracle):
    """against the oracle's full distance matrix: group g's rows are the k smallest of min over its sub-queries"""
    idx, C = gauss
    rng = np.random.default_rng(37)
    n, k, fetch_k = 1500, 10, 10
    Cs = np.ascontiguousarray(C[:n])
    Q = queries_near(rng, Cs, 6)
    offs = [0, 2, 6]
    dist, rows = oracle.topk_search(Cs, Q, n)
    full = np.empty((6, n))
    np.put_along_axis(full, rows, dist, axis=1)
    with pkg.Mi355Index(D) as small:
        small.add(Cs)
        got = small.search_groups(Q, offs, k, fetch_k)
    for g in range(2):
        best = full[offs[g]:offs[g + 1]].min(axis=0)
        order = np.lexsort((np.arange(n), best))
        top = best[order[:k + 1]]
        assert np.unique(top).size == k + 1   # distinct: the cut at k and the order inside it are unambiguous
        assert np.array_equal(got[1][g], order[:k])
        assert np.array_equal(got[0][g].view(np.uint64), top[:k].view(np.uint64))


def test_search_refusals_and_stats(pkg, gauss):
    idx, C = gauss
    Q = np.ascontiguousarray(C[:6])
    idx.reset_stats()
    for offs, k, fetch_k, code in (([0, 6], 0, 5, E_INVALID), ([0, 6], 5, 0, E_INVALID), ([0, 6], 5, -1, E_INVALID),
                                   ([1, 6], 5, 5, E_INVALID), ([0, 4, 2, 6], 5, 5, E_INVALID),
                                   ([0, 6], 5, 1025, E_UNSUPPORTED), ([0, 6], 5, 1024, E_UNSUPPORTED),
                                   ([0, 3, 6], 4097, 1024, E_UNSUPPORTED)):
        with pytest.raises(pkg.NativeError) as e:
            idx.search_groups(Q, offs, k, fetch_k)
        assert e.value.code == code, (offs, k, fetch_k)
    with pytest.raises(ValueError):
        idx.search_groups(Q, [0, 5], 5)                      # offsets that do not end at the number of queries
    assert idx._lib.mi355dr_search_groups(idx._h, None, None, -1, 5, 5, None, None, None) == E_INVALID
    offs = np.array([0, 6], dtype=np.int32)
    op = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert idx._lib.mi355dr_search_groups(idx._h, None, op, 1, 5, 5, None, None, None) == E_INVALID   # null buffers, work to do
    assert idx._lib.mi355dr_search_groups(idx._h, None, None, 0, 5, 5, None, None, None) == 0         # G = 0: a no-op
    d, r, c = idx.search_groups(np.empty((0, D), np.float32), [0], 5)
    assert d.shape == (0, 5) and c.shape == (0,)
    assert (idx.stat("group_searches"), idx.stat("group_subqueries"), idx.stat("groups_merged")) == (0, 0, 0)
    check_search(idx, Q, [0, 2, 6], 5, 4)
    assert (idx.stat("group_searches"), idx.stat("group_subqueries"), idx.stat("groups_merged")) == (1, 6, 2)
