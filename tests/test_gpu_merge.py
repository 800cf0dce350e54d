"""The shard merge (k_merge_topk in csrc/k_select.h, launched by launch_merge in csrc/mi355dr.hip) over its whole shape
range -- both launch widths, sorts of one to sixteen trips of the workgroup, no padding slots, the 4096-entry limit -- and
over tie runs, irregular tails, short lists, signed zeros and extremes, against a plain restatement of the total order.
The same restatement checks the product's host path, autorag_research_amd.sharded.merge_topk_host."""

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROW0 = 2**33  # global rows beyond int32 (and beyond uint32)
NAN_BITS = np.float64(np.nan).view(np.int64)

# (world, B, k)
SHAPES = [
    (1, 5, 1),       # world 1, k 1
    (2, 1, 1),
    (1, 3, 1024),    # world 1 at the largest k
    (8, 37, 16),     # 128 entries: the last shape on 64 threads, no padding slots
    (3, 37, 43),     # 129 entries: the first shape on 256 threads
    (8, 9, 100),     # np = 1024: four trips of the workgroup per sort stage
    (7, 4, 585),     # 4095 entries
    (4, 3, 1024),    # 4096 entries
    (8, 2, 512),     # 4096 entries
    (4096, 2, 1),    # 4096 entries from 4096 ranks
    (16, 1030, 10),  # more queries than one search block
]
MODES = ["random", "one_value", "few_values", "nan_tails", "short_lists", "extremes", "neg_zero", "pos_zero"]
BIG_B_MODES = ["random", "few_values", "short_lists"]  # (16, 1030, 10): the reference is Python's sorted, query by query


def merge_reference(dist_all, rows_all, k):
    """[world, B, k] -> [B, k]: the entries with a row, by (NaN last, distance, row); the first k; NaN / -1 behind them"""
    world, B, _ = dist_all.shape
    out_d = np.full((B, k), np.nan)
    out_r = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        ents = [(float(d), int(r)) for d, r in zip(dist_all[:, b].ravel(), rows_all[:, b].ravel()) if r >= 0]
        ents = sorted(ents, key=lambda e: (math.isnan(e[0]), 0.0 if math.isnan(e[0]) else e[0], e[1]))[:k]
        for s, (d, r) in enumerate(ents):
            out_d[b, s], out_r[b, s] = d, r
    return out_d, out_r


def shard_lists(mode, world, B, k, seed=0):
    """What `world` shards' searches would deliver for B queries: every list sorted under the total order, -1 padding at
    its tail, rows unique across the shards of a query and dealt out at random (row order is not shard order)."""
    rng = np.random.default_rng([seed, world, B, k, MODES.index(mode)])
    n = world * k
    rows = ROW0 + 3 * np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int64) + rng.integers(0, 3, size=(B, n))
    if mode == "random":
        d = rng.standard_normal((B, n))  # distinct
    elif mode == "one_value":
        d = np.full((B, n), 0.25)  # the result is the k smallest rows
    elif mode == "few_values":
        d = rng.choice(np.array([0.125, 0.5, 0.75, 1.5])[: int(rng.integers(3, 5))], size=(B, n))  # tie runs across the k cut
    elif mode == "nan_tails":
        d = rng.choice([0.5, 1.0, 2.0], size=(B, n)) + rng.integers(0, 2, size=(B, n)) * rng.random((B, n))
        d[rng.random((B, n)) < 0.3] = np.nan  # irregular rows: behind every number, by row, ahead of padding
    elif mode == "short_lists":
        d = rng.random((B, n))
        for b in range(B):
            # even queries: fewer than k valid entries over all shards (query 0: none); odd ones: padding, but k or more valid
            m = 0 if b == 0 else int(rng.integers(0, k)) if b % 2 == 0 else int(rng.integers(k, n + 1))
            dead = rng.permutation(n)[m:]
            rows[b, dead] = -1
            d[b, dead] = -7.0 - rng.random(dead.size)  # finite garbage under the padding: must not surface
    elif mode == "extremes":
        # negative distances (inner product), both infinities, subnormals; ties among them break by row
        pool = np.array([-np.inf, -1e300, -3.5, -1.0, -1e-310, -5e-324, 5e-324, 1e-310, 2.0, 1e300, np.inf])
        d = np.where(rng.random((B, n)) < 0.5, rng.choice(pool, size=(B, n)), -np.abs(rng.standard_normal((B, n))))
    else:
        # The inner-product metric returns -0.0 for every zero dot (it negates), cosine returns +0.0.  One query never
        # holds both: an fp32 FMA chain started at +0 never yields -0, so a metric's zero has one sign.  That matters
        # because the kernel orders by key bits (-0.0 ahead of +0.0) while oracle.c and the host merge order numerically
        # (the two zeros tie and the row decides): with a single sign per query the two orders are the same.
        zero = -0.0 if mode == "neg_zero" else 0.0
        d = rng.choice(np.array([zero, zero, 0.5, 1.0]), size=(B, n))
        if mode == "neg_zero":
            d[rng.random((B, n)) < 0.5 * k / n] = -1.5  # about k/2 positive dots per query: the zeros straddle the k cut
    d = d.reshape(B, world, k)
    rows = rows.reshape(B, world, k)
    key = np.where(np.isnan(d), 0.0, d)
    order = np.lexsort((rows, key, np.isnan(d), rows < 0), axis=-1)
    d, rows = np.take_along_axis(d, order, -1), np.take_along_axis(rows, order, -1)
    return np.ascontiguousarray(d.transpose(1, 0, 2)), np.ascontiguousarray(rows.transpose(1, 0, 2))


def assert_same_lists(got_d, got_r, exp_d, exp_r, what):
    assert np.array_equal(got_r, exp_r), what
    nan = np.isnan(exp_d)
    assert np.array_equal(np.isnan(got_d), nan), what
    assert np.array_equal(np.where(nan, NAN_BITS, got_d.view(np.int64)), np.where(nan, NAN_BITS, exp_d.view(np.int64))), what


@pytest.fixture(scope="module")
def idx(native_built):
    import autorag_research_amd as pkg

    with pkg.Mi355Index(8) as index:
        yield index


def device_merges(idx, d, r, k):
    """(merge_topk_device, merge_topk_packed_device) of [world, B, k] lists; every buffer is freed again"""
    world, B, _ = d.shape
    packed = np.ascontiguousarray(np.stack([d.view(np.int64), r], axis=1))  # [world][2][B][k]: what one all-gather delivers
    bufs = [idx.dev_alloc(a.nbytes) for a in (d, r, packed)] + [idx.dev_alloc(B * k * 8) for _ in range(2)]
    pd, pr, pp, od, orr = bufs
    out = []
    try:
        for a, p in ((d, pd), (r, pr), (packed, pp)):
            idx.dev_upload(p, a)
        for call in (lambda: idx.merge_topk_device(pd, pr, world, B, k, od, orr),
                     lambda: idx.merge_topk_packed_device(pp, world, B, k, od, orr)):
            fill = np.full((B, k), 12345.0)  # stale output must not pass for a result
            idx.dev_upload(od, fill)
            idx.dev_upload(orr, fill.view(np.int64))
            call()
            idx.synchronize()
            gd, gr = np.empty((B, k)), np.empty((B, k), dtype=np.int64)
            idx.dev_download(od, gd)
            idx.dev_download(orr, gr)
            out.append((gd, gr))
    finally:
        for p in bufs:
            idx.dev_free(p)
    return out


CASES = [(w, B, k, m) for (w, B, k) in SHAPES for m in (BIG_B_MODES if B > 1000 else MODES)]


@pytest.mark.parametrize("world,B,k,mode", CASES, ids=[f"w{w}-B{B}-k{k}-{m}" for w, B, k, m in CASES])
def test_merge_matches_the_total_order(idx, world, B, k, mode):
    from autorag_research_amd.sharded import merge_topk_host

    d, r = shard_lists(mode, world, B, k)
    exp_d, exp_r = merge_reference(d, r, k)
    (gd, gr), (gd2, gr2) = device_merges(idx, d, r, k)
    assert_same_lists(gd, gr, exp_d, exp_r, "merge_topk_device")
    assert_same_lists(gd2, gr2, exp_d, exp_r, "merge_topk_packed_device")
    hd, hr = merge_topk_host(d, r, k)
    assert_same_lists(hd, hr, exp_d, exp_r, "merge_topk_host")
    if mode == "short_lists":
        assert (exp_r[0] == -1).all() and (B < 3 or (exp_r[2] == -1).any()) and not (gd <= -7.0).any()
    if mode == "neg_zero":
        assert np.signbit(gd[gd == 0]).all()


@pytest.mark.parametrize("mode", MODES)
def test_pack_keeps_bits_and_rows(idx, mode):
    """pack_topk_device: one rank's [B, k] lists -> [2][B][k], plane 0 the distance bits (the sign of zero and NaN included),
    plane 1 the rows"""
    world, B, k = 3, 37, 43
    d, r = shard_lists(mode, world, B, k, seed=1)
    pd, pr, one = idx.dev_alloc(B * k * 8), idx.dev_alloc(B * k * 8), idx.dev_alloc(2 * B * k * 8)
    try:
        idx.dev_upload(pd, d[1])
        idx.dev_upload(pr, r[1])
        idx.pack_topk_device(pd, pr, B, k, one)
        idx.synchronize()
        got = np.empty((2, B, k), dtype=np.int64)
        idx.dev_download(one, got)
    finally:
        for p in (pd, pr, one):
            idx.dev_free(p)
    assert np.array_equal(got[0], d[1].view(np.int64)) and np.array_equal(got[1], r[1])
    if mode == "neg_zero":
        assert (got[0] == np.float64(-0.0).view(np.int64)).any()


def test_merge_limits(idx):
    """above 4096 entries the merge refuses (no launch); no queries is no work"""
    import autorag_research_amd as pkg

    p = idx.dev_alloc(5 * 1024 * 8)
    try:
        for world, k in ((5, 1024), (4097, 1)):
            with pytest.raises(pkg.NativeError, match="4096"):
                idx.merge_topk_device(p, p, world, 1, k, p, p)
            with pytest.raises(pkg.NativeError, match="4096"):
                idx.merge_topk_packed_device(p, world, 1, k, p, p)
        idx.merge_topk_device(p, p, 4, 0, 10, p, p)
        idx.merge_topk_packed_device(p, 4, 0, 10, p, p)
        idx.synchronize()
    finally:
        idx.dev_free(p)
