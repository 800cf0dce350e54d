"""Reference of the speculative pass's model threshold, restated in numpy for the tests.

What the device does (csrc/screen_hits.h screen_emit_slab_max, csrc/k_select.h k_prune thr_only, csrc/mi355dr.hip spec_model):

  per query and 64-row slab of the sample   s1 = sum v,  s2 = sum v^2   in float32, over the slab's values v that are not NaN;
      bf16 screen: v = the screen value;  int8 screen: v = fl((float)acc * m), m = fl(S_g S_q) -- the screen value WITHOUT the
      group's share e_g kq of the bound;
  per query   mean = (sum s1) / rows,  var = (sum s2) / rows - mean^2  in float64 -- rows is the SAMPLE's size, whatever the sums
      left out;  t = (float)(mean + sqrt(max(var, 0)) * (double)(float)zq);
      model = screen_threshold(metric, distance of a row of screen value t);
      thr_used = model if rigorous < model < +inf else rigorous  (a query without a rigorous threshold keeps -inf);
  zq = Phi^-1(1 - m(k) / size) + spec_shift_milli / 1000.

SUMMATION ORDER AND ITS BOUND.  A lane of the wave holds 32 of a slab's 64 values and adds them one after the other (s1 += v;
s2 = fma(v, v, s2): one rounding per step), then adds its partner lane's sum: every term passes through at most 32 roundings,
each of relative size <= u = 2^-24.  The standard bound for any order of n terms is |fl(sum) - sum| <= gamma_(n-1) sum |term|,
gamma_j = j u / (1 - j u); with n = 64, gamma_63 < 64 u.  So per slab

    |s1 - sum v| <= 64 * 2^-24 * sum |v|,      |s2 - sum v^2| <= 64 * 2^-24 * sum v^2

(v^2 is exact inside the fma, and exact in float64 here: 24-bit significands).  Nothing is fitted: `TERMS` is the slab's size.
"""

import math
from statistics import NormalDist

import numpy as np

SLAB = 64
TERMS = SLAB
U32 = 2.0 ** -24


def slab_sums(V):
    """V float64 [B, rows] (rows a multiple of 64), NaN = left out -> float64 (s1, s2, abs1) [B, rows / 64] each: the sums of the
    values, of their squares, of their magnitudes"""
    B, rows = V.shape
    assert rows % SLAB == 0
    v = np.where(np.isnan(V), 0.0, V).reshape(B, rows // SLAB, SLAB)
    return v.sum(axis=2), (v * v).sum(axis=2), np.abs(v).sum(axis=2)


def check_moments(moments, V):
    """the device's per-slab sums [B, slabs, 2] against the float64 sums of the terms V; returns the worst deviation of each sum
    as a fraction of its bound"""
    s1, s2, a1 = slab_sums(V)
    assert moments.shape == s1.shape + (2,)
    got1, got2 = moments[:, :, 0].astype(np.float64), moments[:, :, 1].astype(np.float64)
    tol1, tol2 = TERMS * U32 * a1, TERMS * U32 * s2
    bad1, bad2 = np.abs(got1 - s1) > tol1, np.abs(got2 - s2) > tol2
    assert not bad1.any(), f"sum: {int(bad1.sum())} slabs off, first (query, slab) {np.argwhere(bad1)[0]}: {got1[bad1][0]} vs {s1[bad1][0]}"
    assert not bad2.any(), f"sum of squares: {int(bad2.sum())} slabs off, first (query, slab) {np.argwhere(bad2)[0]}"
    with np.errstate(invalid="ignore", divide="ignore"):
        w1 = np.nanmax(np.where(tol1 > 0, np.abs(got1 - s1) / tol1, 0.0))
        w2 = np.nanmax(np.where(tol2 > 0, np.abs(got2 - s2) / tol2, 0.0))
    return float(w1), float(w2)


def i8_terms(R, m, ek):
    """int8 screen.  R float32 [B, rows]: the dense screen values fl(fma((float)acc, m, ek)) (NaN: row outside the shadow);
    m, ek float32 [B, rows]: fl(S_g S_q) and fl(e_g kq) as the kernels form them.  Recovers the integer accumulator and returns
    the kernel's term fl((float)acc * m) as float64 [B, rows] (NaN where R is), and the accumulators.
    |R - (acc m + ek)| <= 2^-24 |R| (one rounding), so (R - ek) / m lies within 2^-24 |R| / m of the integer -- asserted, and
    asserted to identify it (< 1/4).  m = 0 (a query the screen cannot rank: its image is all zero): the term is 0."""
    R64, m64, ek64 = R.astype(np.float64), m.astype(np.float64), ek.astype(np.float64)
    ok = ~np.isnan(R64)
    live = ok & (m64 > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.where(live, (R64 - ek64) / m64, 0.0)
        slack = np.where(live, U32 * np.abs(R64) / m64, 0.0) + 1e-9 * (1.0 + np.abs(x))
    acc = np.rint(x)
    assert (slack < 0.25).all(), "the accumulator cannot be told from its neighbours"
    off = np.abs(x - acc) > slack
    assert not off.any(), f"{int(off.sum())} values are not fl(acc m + ek) for an integer acc: first {np.argwhere(off)[0]}, acc ~ {x[off][0]}"
    dead = ok & ~live
    assert np.array_equal(R[dead], ek[dead]), "m = 0: the value is the bound term alone"
    assert (np.abs(acc) < 2 ** 24).all()  # ((float)acc is exact)
    term = (acc.astype(np.float32) * m.astype(np.float32)).astype(np.float64)  # one float32 product, as the kernel's
    return np.where(ok, term, np.nan), acc


# ---- the published threshold ----------------------------------------------------------------------------------------------------
def float_below(x):
    """dev_common.h float_below: the next float32 below x (NaN and -inf stay)"""
    x = np.float32(x)
    if np.isnan(x) or x == -np.inf:
        return x
    u = int(x.view(np.uint32))
    if x > 0:
        u -= 1
    elif x < 0:
        u += 1
    else:
        u = 0x80000001
    return np.uint32(u).view(np.float32)


def screen_threshold(metric, dist_k, E, nq):
    """k_select.h screen_threshold: double arithmetic, one rounding to float32, one step down"""
    with np.errstate(over="ignore", invalid="ignore"):
        if metric == "cosine":
            return float_below(np.float32((1.0 - dist_k) - float(E)))
        u = -dist_k / math.sqrt(float(nq))
        return float_below(np.float32(u - abs(u) * 4e-6 - float(E)))


def model_stats(moments, rows):
    """(mean, sd) float64 [B] of the device's moments [B, slabs, 2], reduced in float64, the divisor the sample's size"""
    mean = moments[:, :, 0].astype(np.float64).sum(axis=1) / rows
    var = moments[:, :, 1].astype(np.float64).sum(axis=1) / rows - mean * mean
    return mean, np.sqrt(np.maximum(var, 0.0))


def model_threshold(metric, mean, sd, zq, E, nq):
    """one query's model threshold from its float64 mean and sd, zq as the host computed it (rounded to float32 here as there)"""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.float32(mean + sd * float(np.float32(zq)))
    dist_t = 1.0 - float(t) if metric == "cosine" else -float(t) * math.sqrt(float(nq))
    return screen_threshold(metric, dist_t, E, nq)


def published(rigorous, model):
    """thr_used of a query WITH a rigorous threshold: the model where it is above it and neither NaN nor +inf"""
    return model if (model > rigorous and model < np.inf) else np.float32(rigorous)


def zq_reference(m, n, shift_milli=0):
    return NormalDist().inv_cdf(1.0 - m / n) + shift_milli / 1000.0


def ulps(a, b):
    """distance of two float32 arrays in units in the last place (0 for two equal infinities; NaN against NaN: 0)"""
    def key(x):
        u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
        return np.where(u >> 31 != 0, -(u & 0x7FFFFFFF), u)
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    d = np.abs(key(a) - key(b))
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    return np.where(both_nan, 0, np.where(one_nan, np.iinfo(np.int64).max, d))


# ---- the kernel's summation, emulated (CPU tests: the checks above must reject what they are meant to reject) --------------------
def emulate_slab_moments(V32):
    """float32 [B, rows] terms (NaN: left out) -> [B, slabs, 2] float32, summed as screen_emit_slab_max sums them: a lane of half
    h holds rows 32 i + 4 h + (r & 3) + 8 (r >> 2), i = 0, 1, r = 0 .. 15, in that order, then the two halves are added"""
    B, rows = V32.shape
    v = V32.reshape(B, rows // SLAB, SLAB)
    half = []
    for h in (0, 1):
        s1 = np.zeros(v.shape[:2], dtype=np.float32)
        s2 = np.zeros(v.shape[:2], dtype=np.float64)
        for i in (0, 1):
            for r in range(16):
                x = v[:, :, 32 * i + 4 * h + (r & 3) + 8 * (r >> 2)]
                ok = ~np.isnan(x)
                x0 = np.where(ok, x, np.float32(0))
                s1 = np.where(ok, s1 + x0, s1).astype(np.float32)
                # fma: the product is exact in float64 (24-bit operands); the sum is rounded to float64 and then to float32 -- a
                # second rounding the device does not have, which the bound above covers like the first
                s2 = np.where(ok, (x0.astype(np.float64) * x0.astype(np.float64) + s2).astype(np.float32), s2).astype(np.float64)
        half.append((s1, s2.astype(np.float32)))
    out = np.empty(v.shape[:2] + (2,), dtype=np.float32)
    out[:, :, 0] = half[0][0] + half[1][0]
    out[:, :, 1] = half[0][1] + half[1][1]
    return out
