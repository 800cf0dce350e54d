"""Every hit of the persistent screen kernels (k_screen_stream, k_screen256c, k_screen_rq) against a reference.

Mi355Index.debug_screen_hits runs ONE production screen launch over a row range of any length with the caller's thresholds
and returns the raw candidate lists plus the kernel launch_screen chose.  Each case below

  * builds R[q, row], the dense values of the TILE kernel k_screen over the whole range (the hook at thr = -inf in slices of
    2048 rows, default small_chunk_rows, screen_stream = 0) -- the one kernel test_gpu_kernels.py already value-checks --
    and anchors R to the float64 emulations of screen_ref.py on three slices (first, middle, ragged last);
  * runs the kernel under test once over the range with thr[q] = the 99.5 % quantile of R[q, :] and checks EVERY pair:
      1. the launch took the kernel the case is meant for;
      2. every entry is in range and no (query, row) appears twice;
      3. every emitted value is bit-identical to R (int8: the int32 accumulator is exact and every path forms the value by
         one fmaf((float)acc, S_g S_q, e_g kq); bf16: all four kernels issue v_mfma_f32_32x32x16_bf16 over K ascending, rows
         as A, queries as B, from a zero accumulator -- k_screen.h, k_screen_stream.h, k_screen256c.h, k_screen_rq.h);
      4. every pair with R >= thr (float32 compare) that is in the shadow is emitted;
      5. nothing below the threshold is emitted (see I8_SLACK for the int8 queue kernels).

Data: Gaussian rows cut at +-2.5 sigma, times uniform(0.1, 10) norms.  Every fourth group of 32 rows holds one row with one
or two components raised to 5.5 / sqrt(d) of its norm: that group's int8 step is >= 1.5 x its neighbours' (asserted), so a
kernel that applies a neighbouring group's or tile's (S_g, e_g) to a block is off by half the value, not by a few per cent.
(The cut is what leaves room for that: a row is "loose" -- outside the int8 shadow -- from 6 / sqrt(d) up, and plain
Gaussian groups already peak at 4 ... 4.8 / sqrt(d).)  Three rows with one outlier component (loose) and one zero row lie
inside the range and must never come out as hits; rows just outside the range are copies of the queries (cosine 1): they
would be hits if a kernel did not clip at the range.

I8_SLACK.  The int8 queue kernels re-test a hit lane's accumulators against the integer threshold i8_block_threshold(th, m, ek)
(dev_common.h), m = S_g S_q, ek = e_g kq:  thi = floor(x - 4.8e-7 |x| - 1.2e-7 |th| r - 2), r = rcp(m), x = fl((th - ek) r).
An emitted accumulator has acc >= thi > x - 4.8e-7 |x| - 1.2e-7 |th| r - 3; times m, with x m = (th - ek)(1 + delta),
|delta| < 3.2e-7 (rcp 1 ulp, two roundings) and r m < 1 + 1.3e-7:
    acc m + ek > th - 3 m - 8e-7 |th - ek| - 1.3e-7 |th|,
and the stored value is that rounded once more (6e-8 relative).  So no emitted value lies below
    thr - (3 m + 1e-6 (|thr - ek| + |thr|)),
three accumulator units and a few ulps.  The number of emitted values below thr itself is printed per case (a measurement).
"""

import time

import numpy as np
import pytest
from screen_ref import cos64, e64_bf16, e64_i8

pytestmark = pytest.mark.gpu

K_TILE, K_STREAM, K_256C, K_RQ = 0, 1, 2, 3
KERNEL_NAME = {K_TILE: "k_screen", K_STREAM: "k_screen_stream", K_256C: "k_screen256c", K_RQ: "k_screen_rq"}
ST_OVERFLOW = 1
CAP = 2048
SLICE = 2048   # rows per reference launch (<= the lists' capacity: at thr = -inf every row is an entry)
CUT = 2.5      # the Gaussian components are cut here
PEAK_Z = 5.5   # |component| sqrt(d) / |row| of a peaky row (loose from 6 up: dev_common.h kI8Z)
GROUP = 32


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def _raise_components(C, rows, cols, p):
    """set C[rows[i], cols[i, :]] so that each is p of its row's norm (the other components stay)"""
    sub = C[rows].astype(np.float64)
    ar = np.arange(len(rows))[:, None]
    sign = np.where(sub[ar, cols] < 0, -1.0, 1.0)
    sub[ar, cols] = 0.0
    rest = (sub * sub).sum(axis=1)
    x = p * np.sqrt(rest / (1.0 - cols.shape[1] * p * p))
    C[rows[:, None], cols] = (sign * x[:, None]).astype(np.float32)


def make_case(n_index, d, B, lo, n, seed):
    """(C, Q, planned): the corpus, the queries and the planned rows outside the int8 shadow (three loose, one zero; the zero
    row is last) -- all inside [lo, lo + n)."""
    rng = np.random.default_rng(seed)
    hi = lo + n
    C = rng.standard_normal((n_index, d), dtype=np.float32)
    np.clip(C, -CUT, CUT, out=C)
    Q = rng.standard_normal((B, d), dtype=np.float32)
    groups = np.arange(1, n_index // GROUP, 4)
    peaky = groups * GROUP + 5
    ncomp = 2 if d >= 128 else 1
    cols = (7 * groups[:, None] + 13 * np.arange(ncomp)[None, :]) % d
    _raise_components(C, peaky, cols, PEAK_Z / np.sqrt(d))
    loose = np.array([lo + 70, lo + (n // 2) // GROUP * GROUP + 9, hi - 3 if (hi - 3) % GROUP != 5 else hi - 4])
    zero = lo + 100
    assert not np.isin(np.append(loose, zero), peaky).any() and len({*loose, zero}) == 4 and hi - 4 > lo + 100
    _raise_components(C, loose, np.full((3, 1), 3), min(0.97, 8.0 / np.sqrt(d)))
    C *= rng.uniform(0.1, 10, size=(n_index, 1)).astype(np.float32)
    C[zero] = 0.0
    nb, na = min(B, 32, lo), min(B, 32, n_index - hi)   # rows right outside the range: the queries themselves
    if nb:
        C[lo - nb:lo] = 2.0 * Q[:nb]
    if na:
        C[hi:hi + na] = 3.0 * Q[:na]
    return C, Q, np.append(loose, zero)


def check_peaky_groups(idx, Q, lo, n):
    """the int8 steps of the peaky groups stand >= 1.5 x above both neighbours' (groups whole inside the range)"""
    g0, g1 = lo // GROUP, (lo + n) // GROUP
    _, _, step, _ = idx.debug_i8_state(Q[:1], g0, g1 - g0)
    g = np.arange(g0 + 1, g1 - 1)
    g = g[g % 4 == 1] - g0
    assert len(g) >= (g1 - g0) // 4 - 1
    assert (step[g] >= 1.5 * np.maximum(step[g - 1], step[g + 1])).all()


def tile_reference(idx, Q, lo, n, absent, i8):
    """R[q, row - lo]: the tile kernel's value of every pair of the range (NaN for the rows `absent`: outside the shadow)"""
    B = len(Q)
    idx.set_option("screen_stream", 0)
    R = np.full((B, n), np.nan, dtype=np.float32)
    thr = np.full(B, -np.inf, dtype=np.float32)
    for s in range(0, n, SLICE):
        m = min(SLICE, n - s)
        h = idx.debug_screen_hits(Q, lo + s, m, thr, CAP)
        assert h["kernel"] == K_TILE
        # (int8: rows outside the shadow are entries with a stale accumulator, dropped by the wrapper; bf16: the zero row's
        # NaN image passes no threshold, -inf included)
        gone = int(((absent >= lo + s) & (absent < lo + s + m)).sum()) if i8 else int(lo + s <= absent[-1] < lo + s + m)
        assert (h["count"] == (m if i8 else m - gone)).all() and not h["status"].any()
        assert (h["dropped"] == (gone if i8 else 0)).all()
        col = h["row"].astype(np.int64) - lo
        assert ((col >= s) & (col < s + m)).all()
        R[h["q"], col] = h["val"]
        assert np.count_nonzero(~np.isnan(R[:, s:s + m])) == len(col), "a pair twice, or a NaN value"
    present = ~np.isnan(R)
    missing_cols = np.flatnonzero(~present.all(axis=0))
    want = np.sort(absent - lo) if i8 else absent[-1:] - lo
    assert np.array_equal(missing_cols, want) and not present[:, want].any(), "every pair outside the planned rows is present"
    return R


def anchor_to_e64(idx, Q, C, R, lo, n, i8):
    """R against the float64 emulation on the first slice, one from the middle and the ragged last one"""
    E = idx.debug_screen_bound(Q).astype(np.float64)
    for s in sorted({0, (n // SLICE // 2) * SLICE, (n - 1) // SLICE * SLICE}):
        m = min(SLICE, n - s)
        sub = C[lo + s:lo + s + m]
        t = R[:, s:s + m].astype(np.float64)
        ok = ~np.isnan(t).all(axis=0)
        cos = cos64(Q, sub)[:, ok]
        if i8:
            g0 = (lo + s) // GROUP
            sq, kq, step, err = idx.debug_i8_state(Q, g0, (lo + s + m + GROUP - 1) // GROUP - g0)
            gi = np.arange(lo + s, lo + s + m) // GROUP - g0
            ref, unit = e64_i8(Q, sub, sq, kq, step[gi], err[gi])
            dlt = np.abs(t - ref)[:, ok]
            assert (dlt <= 4 * 127 * unit[:, ok] + 1e-6).all()
            assert dlt.mean() < 1e-5
            assert (cos <= t[:, ok] + E[:, None]).all()
        else:
            dlt = np.abs(t - e64_bf16(Q, sub))[:, ok]
            assert dlt.max() < 2e-3
            assert dlt.mean() < 2e-5
            assert (np.abs(t[:, ok] - cos) <= E[:, None]).all()


def quantile_thresholds(R, qtl):
    n_ok = R.shape[1] - int(np.isnan(R[0]).sum())
    kth = int(qtl * n_ok)
    return np.ascontiguousarray(np.partition(R, kth, axis=1)[:, kth])   # (NaN sorts last)


def check_entries(h, R, lo):
    """assertions 2 and 3 for every entry of the lists; returns (query, column) of the entries"""
    B, n = R.shape
    q = h["q"].astype(np.int64)
    col = h["row"].astype(np.int64) - lo
    assert ((q >= 0) & (q < B)).all()
    assert ((col >= 0) & (col < n)).all(), "a row outside the range"
    key = q * n + col
    assert len(np.unique(key)) == len(key), "a (query, row) pair twice"
    ref = R[q, col]
    assert not np.isnan(ref).any(), "a row outside the shadow was emitted"
    assert np.array_equal(h["val"].view(np.uint32), ref.view(np.uint32)), "a value differs from the tile kernel's"
    return q, col


def i8_slack(idx, Q, lo, n, q, col, thr):
    """I8_SLACK of every entry (module docstring)"""
    g0 = lo // GROUP
    sq, kq, step, err = idx.debug_i8_state(Q, g0, (lo + n + GROUP - 1) // GROUP - g0)
    gi = (col + lo) // GROUP - g0
    m = (step[gi] * sq[q]).astype(np.float64)     # float32 products, as the kernels form them
    ek = (err[gi] * kq[q]).astype(np.float64)
    th = thr[q].astype(np.float64)
    return 3.0 * m + 1e-6 * (np.abs(th - ek) + np.abs(th))


def run_sparse(pkg, *, dtype, d, B, n_index, lo, n, kernel, seed, options=()):
    t0 = time.perf_counter()
    i8 = dtype == "i8"
    C, Q, absent = make_case(n_index, d, B, lo, n, seed)
    with pkg.Mi355Index(d) as idx:
        idx.set_option("screen_dtype", dtype)
        idx.add(C)
        if i8:
            assert idx.stat("loose_rows") == len(absent)
            check_peaky_groups(idx, Q, lo, n)
        R = tile_reference(idx, Q, lo, n, absent, i8)
        anchor_to_e64(idx, Q, C, R, lo, n, i8)
        thr = quantile_thresholds(R, 0.995)
        idx.set_option("screen_stream", 1)
        idx.set_option("small_chunk_rows", 0)
        for key, value in options:
            idx.set_option(key, value)
        idx.reset_stats()
        h = idx.debug_screen_hits(Q, lo, n, thr, CAP)
        rq_launches = idx.stat("screen_rq_launches")
        assert h["kernel"] == kernel, KERNEL_NAME[h["kernel"]]                                    # 1
        assert (rq_launches > 0) == (kernel == K_RQ)
        assert not (h["status"] & ST_OVERFLOW).any() and (h["count"] <= CAP).all()
        assert not h["dropped"].any(), "a row outside the int8 shadow was emitted"
        q, col = check_entries(h, R, lo)                                                          # 2, 3
        emitted = np.zeros(R.shape, dtype=bool)
        emitted[q, col] = True
        with np.errstate(invalid="ignore"):
            expected = R >= thr[:, None]
        assert not (expected & ~emitted).any(), "a pair at or above its threshold is missing"     # 4
        below = h["val"] < thr[q]                                                                 # 5
        if i8 and kernel in (K_256C, K_RQ):
            assert (h["val"].astype(np.float64) >= thr[q].astype(np.float64) - i8_slack(idx, Q, lo, n, q, col, thr)).all()
        else:
            assert not below.any()
    print(f"SCREEN_HITS {KERNEL_NAME[kernel]} {dtype} d={d} B={B} n={n} lo={lo} {dict(options)}: pairs={B * n} "
          f"hits={len(q)} per_query={len(q) / B:.1f} below_thr={int(below.sum())} wall={time.perf_counter() - t0:.2f}s")


# ---- k_screen_rq --------------------------------------------------------------------------------------------------------
# B = 1024: 4 query tiles, 256 workgroups, 64 tiles between two visits.  n = 20 000: 157 tiles of 128 rows, 2 to 3 visits.
@pytest.mark.parametrize("d,options", [
    (128, ()), (200, ()), (384, ()), (512, ()), (640, ()), (768, ()),          # KS = 1 .. 6 (d = 200: padded to 256)
    (768, (("screen_rq_split_tests", 0),)),
    (384, (("screen_flush_sync", 0),)),
])
def test_rq_every_form_over_several_visits(pkg, d, options):
    run_sparse(pkg, dtype="i8", d=d, B=1024, n_index=20_000, lo=0, n=20_000, kernel=K_RQ, seed=1000 + d, options=options)


@pytest.mark.parametrize("d", [128, 768])
def test_rq_records_ring_wraps(pkg, d):
    """528 tiles: tiles 512 .. 527 bring 16 workgroups a ninth visit (kRqRecSlots = 8), the others stop at eight; ragged end"""
    run_sparse(pkg, dtype="i8", d=d, B=1024, n_index=67_500, lo=0, n=67_500, kernel=K_RQ, seed=2000 + d)


EDGE = dict(n_index=21_500, lo=2_560, n=17_907)   # the end is no multiple of 32, and live rows lie behind it


@pytest.mark.parametrize("B,options", [
    (129, ()),                        # one query tile, queries 129 .. 255 are padding
    (600, ()),                        # three query tiles
    (1024, ()),
    (1024, (("screen_drift", 0),)),
    (1024, (("screen_drift", 1),)),
])
def test_rq_range_edges(pkg, B, options):
    run_sparse(pkg, dtype="i8", d=384, B=B, kernel=K_RQ, seed=3000 + B, options=options, **EDGE)


# ---- k_screen256c ---------------------------------------------------------------------------------------------------------
# n = 70 000: 274 tiles of 256 rows, up to five visits -- its four record slots wrap
@pytest.mark.parametrize("d", [64, 128, 200])
def test_256c_bf16(pkg, d):
    run_sparse(pkg, dtype="bf16", d=d, B=1024, n_index=70_000, lo=0, n=70_000, kernel=K_256C, seed=4000 + d)


def test_256c_int8_when_rq_is_off(pkg):
    run_sparse(pkg, dtype="i8", d=128, B=1024, n_index=70_000, lo=0, n=70_000, kernel=K_256C, seed=4500,
               options=(("screen_rq", 0),))


def test_256c_int8_seven_ksteps(pkg):
    """d = 896: 7 K-steps, where k_screen_rq has no form"""
    run_sparse(pkg, dtype="i8", d=896, B=1024, n_index=20_000, lo=0, n=20_000, kernel=K_256C, seed=4600)


@pytest.mark.parametrize("B", [129, 600])
def test_256c_bf16_range_edges(pkg, B):
    run_sparse(pkg, dtype="bf16", d=384, B=B, kernel=K_256C, seed=4700 + B, **EDGE)


# ---- k_screen_stream --------------------------------------------------------------------------------------------------------
def stream_or_tile(dtype, d, B):
    """launch_screen's rule for B <= 64: the streaming form while the resident query image (32 or 64 rows) fits 48 KiB --
    the bf16 image of 64 queries at d = 768 is 96 KiB, so those two combinations stay with the tile kernel (asserted: the
    case then checks that the launch over the long range falls back as designed)"""
    row_bytes = -(-d * (1 if dtype == "i8" else 2) // 128) * 128
    return K_STREAM if (32 if B <= 32 else 64) * row_bytes <= 48 * 1024 else K_TILE


# n = 70 000: 547 tiles over 256 workgroups, two or three visits each, more stages than the ring's six
@pytest.mark.parametrize("dtype", ["bf16", "i8"])
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("B", [1, 32, 33, 64])
def test_stream_over_several_visits(pkg, dtype, d, B):
    run_sparse(pkg, dtype=dtype, d=d, B=B, n_index=70_000, lo=0, n=70_000, kernel=stream_or_tile(dtype, d, B),
               seed=5000 + d + B)


@pytest.mark.parametrize("dtype", ["bf16", "i8"])
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("B", [1, 32, 33, 64])
def test_stream_range_edges(pkg, dtype, d, B):
    run_sparse(pkg, dtype=dtype, d=d, B=B, kernel=stream_or_tile(dtype, d, B), seed=6000 + d + B, **EDGE)


# ---- the dense regime: the designed, bounded overflow paths -------------------------------------------------------------------
DENSE_N = 2048


@pytest.fixture(scope="module")
def dense_i8(pkg):
    """one small int8 index with its tile-kernel reference for 130 queries (a screen value does not depend on the block size)"""
    d, B, n_index = 128, 130, DENSE_N + 256
    C, Q, absent = make_case(n_index, d, B, 0, DENSE_N, seed=7000)
    with pkg.Mi355Index(d) as idx:
        idx.set_option("screen_dtype", "i8")
        idx.add(C)
        assert idx.stat("loose_rows") == len(absent)
        R = tile_reference(idx, Q, 0, DENSE_N, absent, True)
        anchor_to_e64(idx, Q, C, R, 0, DENSE_N, True)
        R.setflags(write=False)
        yield idx, Q, R, absent


def test_rq_dense_every_block_fills_the_lane_queue(dense_i8):
    """thr = -inf: all 64 lanes of every block are hit lanes, so from a tile's second block on the queue is expanded at the
    test site (lane_queue_flush_small).  Every pair comes out, bit-identical, and nothing is flagged."""
    idx, Q, R, absent = dense_i8
    idx.set_option("screen_stream", 1)
    idx.set_option("small_chunk_rows", 0)
    idx.set_option("screen_rq", 1)
    h = idx.debug_screen_hits(Q, 0, DENSE_N, np.full(len(Q), -np.inf, dtype=np.float32), CAP)
    assert h["kernel"] == K_RQ
    assert not h["status"].any() and (h["count"] == DENSE_N).all() and (h["dropped"] == len(absent)).all()
    q, col = check_entries(h, R, 0)
    assert len(q) == len(Q) * (DENSE_N - len(absent))   # unique and inside the shadow: every such pair is there
    print(f"SCREEN_HITS k_screen_rq i8 dense: pairs={len(Q) * DENSE_N}")


@pytest.mark.parametrize("kernel,B,options", [
    (K_RQ, 130, (("small_chunk_rows", 0), ("screen_rq", 1))),
    (K_TILE, 130, (("small_chunk_rows", 16384), ("screen_stream", 0))),
    (K_STREAM, 40, (("screen_stream", 1),)),
])
def test_short_lists_keep_their_first_entries(dense_i8, kernel, B, options):
    """cap = 16 at thr = -inf: the counter runs past the list, whose 16 entries are valid, distinct and exact"""
    idx, Q, R, _ = dense_i8
    for key, value in options:
        idx.set_option(key, value)
    h = idx.debug_screen_hits(Q[:B], 0, DENSE_N, np.full(B, -np.inf, dtype=np.float32), 16)
    assert h["kernel"] == kernel
    assert (h["count"] > 16).all()
    q, _ = check_entries(h, R[:B], 0)
    assert (np.bincount(q, minlength=B) + h["dropped"] == 16).all()


def test_256c_dense_loss_is_never_silent(pkg):
    """bf16, thr at the 80 % quantile: ~1 600 hits per wave tile (128 rows x 64 queries) against a queue of 320.  For every
    query: kStOverflow is set, or the counter passed the list, or the list is complete -- what complete_block relies on.
    Whatever is in a list is still unique, in range, bit-identical and at or above the threshold."""
    d, B, n = 128, 256, 4096
    C, Q, absent = make_case(n + 256, d, B, 0, n, seed=8000)
    with pkg.Mi355Index(d) as idx:
        idx.set_option("screen_dtype", "bf16")
        idx.add(C)
        R = tile_reference(idx, Q, 0, n, absent, False)
        anchor_to_e64(idx, Q, C, R, 0, n, False)
        thr = quantile_thresholds(R, 0.80)
        idx.set_option("small_chunk_rows", 0)
        h = idx.debug_screen_hits(Q, 0, n, thr, CAP)
    assert h["kernel"] == K_256C
    q, col = check_entries(h, R, 0)
    assert (h["val"] >= thr[q]).all()
    emitted = np.zeros(R.shape, dtype=bool)
    emitted[q, col] = True
    with np.errstate(invalid="ignore"):
        complete = ~((R >= thr[:, None]) & ~emitted).any(axis=1)
    flagged = ((h["status"] & ST_OVERFLOW) != 0) | (h["count"] > CAP)
    assert (flagged | complete).all(), "a query lost a hit without being flagged"
    assert flagged.any(), "the queue never filled: the path under test did not run"
    print(f"SCREEN_HITS k_screen256c bf16 dense: pairs={B * n} flagged={int(flagged.sum())} complete={int(complete.sum())}")
