"""GPU: the model threshold of the speculative one-chunk pass against a reference.

Mi355Index.debug_spec_model runs what a speculative search runs in front of its one chunk -- prepare, the starter screen with
its per-slab sums, the thr_only prune -- and hands back the sums, the rigorous threshold, the published one and zq.  Exactness
of the results never depends on this arithmetic (k_finalize verifies every query), so only a reference can see it go wrong.

REFERENCE OF THE SUMS: the device's own dense screen values of the sample rows (debug_screen_dense in slices of 2048 rows),
summed in float64 per 64-row slab and query.  The screen kernels form a value the same way in every epilogue (bit-identical:
test_gpu_screen_hits.py), so the only difference left is the float32 accumulation, bounded per slab by
64 * 2^-24 * sum |term| (derived in spec_model_ref.py from the kernel's summation order; not tuned).
  bf16: the terms are the values; NaN images (the zero row, the removed row) are left out, every other value is in.
  int8: the kernel sums fl((float)acc * m) WITHOUT the group's e_g kq.  The integer accumulator is recovered from the dense value
        with the device's own S_g, e_g, S_q, kq (float32 products, as the kernels form them), asserted to be an integer to
        rounding, and the term rebuilt in float32 (spec_model_ref.i8_terms): with e_g kq left in, every term is off by ~e_g.
        Rows outside the int8 shadow (loose, removed) have an all-zero image: they add 0, as if left out.

THE PUBLISHED THRESHOLD: a Python mirror of screen_threshold / float_below fed with the float64 reduction of the RETURNED sums and
zq.  The device reduces the 256 slab sums in float64 in another order (differences ~1e-16 relative), rounds t to float32 once
and the threshold once more: the mirror may sit on the other side of a rounding boundary of either -- 2 float32 ulps, as the
issue of this test states.  zq is a double on both sides (bisection on erfc to the last bit against NormalDist.inv_cdf): 1e-9.

AGAINST GROUND TRUTH (cosine): every summed value lies within b of the exact cosine, b = E_q (bf16: |value - cosine| <= E_q,
include/mi355dr.h) or E_q + e_g kq of the row's own group (int8: the term is the screen value minus the group's share) -- asserted element by
element.  With left-out rows counted as 0 on both sides, the mean moves by at most max b; the standard deviation is a seminorm of the vector of values, so an
elementwise error <= b moves it by at most max b as well.  On top: the float32 accumulation bound of the sums, propagated
(d mean <= sum tol1 / rows;  d sd <= (sum tol2 / rows + 2 |mean| d mean) / (2 sd)).

Measured worst deviations (one run, as fractions of the bounds) are in CHANGELOG.md."""

import numpy as np
import pytest
import spec_model_ref as ref
from helpers import MutableOracleIndex
from screen_ref import cos64
from spec_common import B_ALL, GROUP, LOOSE_ROW, NAN_Q, REMOVED_ROW, SAMPLE, SLICE, UPDATED_ROW, ZERO_Q, ZERO_ROW, arm, counters, same
from spec_common import THR_K as K
from spec_common import THR_N as N
from spec_common import threshold_case as make_case

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -4


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


class Cases:
    """one mutated index per (d, metric), and per screen type its references, each computed once"""

    def __init__(self, pkg):
        self.pkg, self.idx, self.data, self.refs = pkg, {}, {}, {}

    def close(self):
        for idx in self.idx.values():
            idx.close()

    def get(self, d, metric, dtype):
        if (d, metric) not in self.idx:
            C, new, Q = make_case(d, 100 + d + (1000 if metric == "ip" else 0))
            idx = self.pkg.Mi355Index(d, metric)
            idx.add(C)
            idx.update_rows([UPDATED_ROW], new[None, :])
            idx.remove_rows([REMOVED_ROW])
            arm(idx)
            now = C.copy()
            now[UPDATED_ROW] = new
            now.setflags(write=False)
            self.idx[d, metric], self.data[d, metric] = idx, (C, new, now, Q)
        idx = self.idx[d, metric]
        C, new, now, Q = self.data[d, metric]
        idx.set_option("screen_dtype", dtype)
        idx.set_option("spec_shift_milli", 0)
        if (d, metric, dtype) not in self.refs:
            self.refs[d, metric, dtype] = self._reference(idx, Q, dtype)
        return idx, now, Q, self.refs[d, metric, dtype]

    @staticmethod
    def _reference(idx, Q, dtype):
        """V [130, SAMPLE]: the kernel's terms from the device's dense values; the hook first: it names the screen the dense
        values then come from"""
        out = idx.debug_spec_model(Q, K)
        i8 = out["i8"]
        assert i8 == (dtype == "auto"), "auto takes the int8 screen on these corpora"
        R = np.concatenate([idx.debug_screen_dense(Q, s, SLICE) for s in range(0, SAMPLE, SLICE)], axis=1)
        absent = np.flatnonzero(np.isnan(R).all(axis=0))
        assert not np.isnan(R[:, np.setdiff1d(np.arange(SAMPLE), absent)]).any(), "a row is there for some queries only"
        E = idx.debug_screen_bound(Q)
        r = {"i8": i8, "R": R, "E": E, "absent": absent}
        if i8:
            assert {LOOSE_ROW, REMOVED_ROW} <= set(absent.tolist()) <= {LOOSE_ROW, REMOVED_ROW, ZERO_ROW}
            sq, kq, step, err = idx.debug_i8_state(Q, 0, SAMPLE // GROUP)
            gi = np.arange(SAMPLE) // GROUP
            m = step[gi][None, :] * sq[:, None]     # float32 products, as the kernels form them
            ek = err[gi][None, :] * kq[:, None]
            assert m.dtype == np.float32 and ek.dtype == np.float32
            V, acc = ref.i8_terms(R, m, ek)
            assert np.abs(acc).max() > 1000, "accumulators of a real dot product"
            r.update(V=V, m=m, ek=ek)
        else:
            assert set(absent.tolist()) == {ZERO_ROW, REMOVED_ROW}
            r["V"] = R.astype(np.float64)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        return r


@pytest.fixture(scope="module")
def cases(pkg):
    c = Cases(pkg)
    yield c
    c.close()


SHAPES = [(d, B, "cosine") for d in (64, 100, 200) for B in (1, 40, B_ALL)] + [(100, 40, "ip"), (64, B_ALL, "ip")]


def regular(Q):
    r = np.ones(len(Q), dtype=bool)
    r[[i for i in (ZERO_Q, NAN_Q) if i < len(Q)]] = False
    return r


@pytest.mark.parametrize("dtype", ["bf16", "auto"])
@pytest.mark.parametrize("d,B,metric", SHAPES)
def test_slab_moments(cases, d, B, metric, dtype):
    """every per-slab sum and sum of squares within the float32 accumulation bound of the kernel's own terms"""
    idx, _, Q, r = cases.get(d, metric, dtype)
    out = idx.debug_spec_model(Q[:B], K)
    assert out["sample_rows"] == SAMPLE and out["moments"].shape == (B, SAMPLE // ref.SLAB, 2) and out["i8"] == r["i8"]
    w1, w2 = ref.check_moments(out["moments"], r["V"][:B])
    print(f"SPEC_MOMENTS d={d} B={B} {metric} {'i8' if r['i8'] else 'bf16'}: worst |s1 - ref| / bound = {w1:.4f}, "
          f"|s2 - ref| / bound = {w2:.4f}")


def expected_thr_used(out, Q, E, metric):
    mean, sd = ref.model_stats(out["moments"], out["sample_rows"])
    nq = (Q.astype(np.float64) ** 2).sum(axis=1)
    want = np.full(len(Q), -np.inf, dtype=np.float32)
    model = np.full(len(Q), np.nan, dtype=np.float32)
    for b in np.flatnonzero(regular(Q)):
        model[b] = ref.model_threshold(metric, mean[b], sd[b], out["zq"], E[b], nq[b])
        want[b] = ref.published(out["thr_rigorous"][b], model[b])
    return want, model, sd


@pytest.mark.parametrize("dtype", ["bf16", "auto"])
@pytest.mark.parametrize("d,B,metric", SHAPES)
def test_published_threshold(cases, d, B, metric, dtype):
    """thr_used == max(rigorous, model of the returned sums) within 2 ulps; zq to 1e-9; irregular queries keep -inf"""
    idx, _, Q, r = cases.get(d, metric, dtype)
    Q = Q[:B]
    out = idx.debug_spec_model(Q, K)
    m = idx._lib.mi355dr_debug_spec_m(K)
    assert m > 0 and abs(out["zq"] - ref.zq_reference(m, len(idx))) <= 1e-9      # (len: removed rows included)
    want, model, _ = expected_thr_used(out, Q, r["E"], metric)
    reg = regular(Q)
    assert np.isfinite(out["thr_rigorous"][reg]).all() and np.isfinite(model[reg]).all()
    assert (out["thr_used"][~reg] == -np.inf).all(), "a query without a rigorous threshold keeps -inf"
    assert (out["thr_rigorous"][~reg] == np.inf).all(), "... and is parked: the screen emits nothing for it"
    worst = int(ref.ulps(out["thr_used"], want).max())
    print(f"SPEC_THRESHOLD d={d} B={B} {metric} {'i8' if r['i8'] else 'bf16'}: worst |thr_used - mirror| = {worst} ulp; "
          f"model above rigorous for {int((model[reg] > out['thr_rigorous'][reg]).sum())} of {int(reg.sum())}")
    assert worst <= 2
    assert (out["thr_used"][reg] >= out["thr_rigorous"][reg]).all()


@pytest.mark.parametrize("dtype", ["bf16", "auto"])
@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_shift_moves_the_model_term_by_one_and_a_half_sd(cases, metric, dtype):
    """spec_shift_milli = +-1500: the same sums, zq moved by exactly 1.5, and the published threshold follows its mirror; where the
    model wins at shift 0 and +1500 the two thresholds differ by 1.5 sd to rounding.  Per side: zq is rounded to float32
    (2^-24 |zq| sd), t is rounded to float32 (2^-24 |t|), the threshold is rounded once and stepped down once (3 * 2^-24 |thr|);
    the inner product's threshold also takes 4e-6 |t| off, which differs by 4e-6 * 1.5 sd between the two."""
    idx, _, Q, r = cases.get(64, metric, dtype)
    reg = regular(Q)
    base = idx.debug_spec_model(Q, K)
    got = {0: base}
    for shift in (1500, -1500):
        idx.set_option("spec_shift_milli", shift)
        out = idx.debug_spec_model(Q, K)
        got[shift] = out
        assert np.array_equal(out["moments"].view(np.uint32), base["moments"].view(np.uint32))
        assert np.array_equal(out["thr_rigorous"].view(np.uint32), base["thr_rigorous"].view(np.uint32))
        assert abs((out["zq"] - base["zq"]) - shift / 1000.0) <= 1e-12
        want, _, _ = expected_thr_used(out, Q, r["E"], metric)
        assert ref.ulps(out["thr_used"], want).max() <= 2
        assert (out["thr_used"][~reg] == -np.inf).all()
    idx.set_option("spec_shift_milli", 0)
    mean, sd = ref.model_stats(base["moments"], SAMPLE)
    wins = reg & (base["thr_used"] > base["thr_rigorous"])
    assert wins.any(), "no query whose model is above its sample's rigorous threshold: the difference below checks nothing"
    mean, sd = mean[wins], sd[wins]
    thr0, thr1 = (got[s]["thr_used"][wins].astype(np.float64) for s in (0, 1500))
    t0, t1 = np.abs(mean + sd * base["zq"]), np.abs(mean + sd * got[1500]["zq"])
    tol = ref.U32 * (sd * (2 * abs(base["zq"]) + 1.5) + t0 + t1 + 3 * np.abs(thr0) + 3 * np.abs(thr1))
    if metric == "ip":
        tol += 4e-6 * 1.5 * sd      # (the threshold takes |u| 4e-6 off u = t)
    print(f"SPEC_SHIFT {metric} {'i8' if r['i8'] else 'bf16'}: worst |d thr - 1.5 sd| / bound = "
          f"{(np.abs(thr1 - thr0 - 1.5 * sd) / tol).max():.4f} over {int(wins.sum())} queries")
    assert (np.abs(thr1 - thr0 - 1.5 * sd) <= tol).all()
    assert (got[-1500]["thr_used"][reg] <= base["thr_used"][reg]).all()


@pytest.mark.parametrize("dtype", ["bf16", "auto"])
@pytest.mark.parametrize("d", [64, 100, 200])
def test_moments_against_exact_cosines(cases, d, dtype):
    """the device's mean and standard deviation within the screen's bound of those of the float64 cosines of the sample"""
    idx, now, Q, r = cases.get(d, "cosine", dtype)
    reg = regular(Q)
    out = idx.debug_spec_model(Q, K)
    mean, sd = ref.model_stats(out["moments"], SAMPLE)
    with np.errstate(invalid="ignore"):
        cos = cos64(Q[reg], now[:SAMPLE])
    included = ~np.isnan(r["V"][reg])
    assert not np.isnan(cos[included]).any()
    x = np.where(included, cos, 0.0)
    E = r["E"][reg].astype(np.float64)
    each = E[:, None] + (np.where(included, r["ek"][reg].astype(np.float64), 0.0) if r["i8"] else 0.0)   # (its own group's e_g kq)
    assert (np.abs(np.where(included, r["V"][reg], 0.0) - x) <= each).all(), "a summed value outside its bound"
    b = np.broadcast_to(each, x.shape).max(axis=1)      # (mean and sd: the largest elementwise bound)
    _, s2, a1 = ref.slab_sums(r["V"][reg])
    d_mean = ref.TERMS * ref.U32 * a1.sum(axis=1) / SAMPLE
    d_sd = (ref.TERMS * ref.U32 * s2.sum(axis=1) / SAMPLE + 2 * np.abs(mean[reg]) * d_mean) / (2 * sd[reg])
    em, es = np.abs(mean[reg] - x.mean(axis=1)), np.abs(sd[reg] - x.std(axis=1))
    print(f"SPEC_TRUTH d={d} {'i8' if r['i8'] else 'bf16'}: worst |mean - exact| / bound = {(em / (b + d_mean)).max():.4f}, "
          f"|sd - exact| / bound = {(es / (b + d_sd)).max():.4f}; bound {b.min():.2e} .. {b.max():.2e}")
    assert (em <= b + d_mean).all() and (es <= b + d_sd).all()


def test_hook_refuses_what_would_not_speculate_and_leaves_the_index_as_it_was(pkg, cases, oracle):
    idx, _, Q, _ = cases.get(64, "cosine", "auto")
    C, new, _, _ = cases.data[64, "cosine"]
    mo = MutableOracleIndex(64)
    mo.add(C)
    mo.update_rows([UPDATED_ROW], new[None, :])
    mo.remove_rows([REMOVED_ROW])
    want = mo.search(Q[:40], K)
    watched = ("spec_passes", "passes", "chunks", "starters", "screen_launches", "screen_rows", "retry_queries",
               "fallback_queries", "spec_miss_queries", "spec_overflow_queries", "spec_suspended", "i8_demoted",
               "candidates", "rescored")      # (the last two: counted on the device by the prunes the hook launches)

    def refused(k=K):
        with pytest.raises(pkg.NativeError) as e:
            idx.debug_spec_model(Q[:40], k)
        assert e.value.code == E_UNSUPPORTED

    idx.reset_stats()
    same(idx.search(Q[:40], K), want)      # (so that the counters the hook must not move are not at zero)
    before = {s: idx.stat(s) for s in watched}
    assert before["spec_passes"] == 1 and before["candidates"] > 0 and before["rescored"] > 0
    idx.debug_spec_model(Q[:40], K)
    idx.debug_spec_model(Q[:40], 2)
    idx.debug_spec_model(Q[:40], 19)
    for k in (1, 20, 24, 100):        # (m(k) = 0, or the wide prune)
        refused(k)
    idx.set_option("speculate", 0)
    refused()
    idx.set_option("speculate", 1)
    idx.set_option("spec_min_rows", N + 1)
    refused()
    idx.set_option("spec_min_rows", N)
    idx.set_option("path", "scan")
    refused()
    idx.set_option("path", "auto")
    assert {s: idx.stat(s) for s in watched} == before
    idx.reset_stats()
    same(idx.search(Q[:40], K), want)
    st = counters(idx)
    print("SPEC_HOOK then search:", st)
    assert st["spec_passes"] == 1 and st["passes"] >= 1
    # suspended speculation is refused too, and the hook does not count the suspension down
    idx.set_option("spec_shift_milli", 1500)
    same(idx.search(Q[:40], K), want)
    assert idx.stat("spec_suspended") == 1
    idx.set_option("spec_shift_milli", 0)
    for _ in range(20):
        refused()
    assert idx.stat("spec_suspended") == 1
    idx.set_option("speculate", 1)      # (re-arms)
    assert idx.stat("spec_suspended") == 0
    idx.debug_spec_model(Q[:40], K)
