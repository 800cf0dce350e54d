"""CPU: the checks of tests/test_gpu_spec_threshold.py can fail.  The starter's sums are emulated in numpy on that test's own
corpus (float32, the kernel's summation order: spec_model_ref.emulate_slab_moments), the reference accepts them, and rejects
each of three perturbed forms: a slab's sums written one slot further, the int8 bound term e_g kq left in the summed value,
and the divisor taken as the number of summed rows instead of the sample's size."""

import numpy as np
import pytest
import spec_model_ref as ref
from screen_ref import e64_bf16, unit_rows64
from spec_common import GROUP, NAN_Q, REMOVED_ROW, SAMPLE, UPDATED_ROW, ZERO_Q, ZERO_ROW
from spec_common import THR_K as K
from spec_common import THR_N as N
from spec_common import threshold_case as make_case


@pytest.fixture(scope="module")
def sample():
    C, new, Q = make_case(64, 164)
    sub = C[:SAMPLE].copy()
    sub[UPDATED_ROW] = new
    Q = Q[[0, 1, 2, ZERO_Q + 2, 129]]    # (regular queries only: the irregular ones have no threshold to check)
    assert ZERO_Q + 2 != NAN_Q and not np.isnan(Q).any() and np.abs(Q).sum(axis=1).all()
    return Q, sub


@pytest.fixture(scope="module")
def bf16_values(sample):
    Q, sub = sample
    V = e64_bf16(Q, sub).astype(np.float32)     # (the zero row: NaN, as its image)
    V[:, REMOVED_ROW] = np.nan
    assert np.isnan(V[:, ZERO_ROW]).all()
    return V


@pytest.fixture(scope="module")
def i8_state(sample):
    """accumulators, m = fl(S_g S_q), ek = fl(e_g kq) and the dense values fl(fma(acc, m, ek)), quantised as dev_common.h says"""
    Q, sub = sample
    qh = unit_rows64(Q)
    with np.errstate(invalid="ignore"):
        ch = np.nan_to_num(unit_rows64(sub))
    sq = (np.abs(qh).max(axis=1) / 127).astype(np.float32)
    step = (np.abs(ch).reshape(-1, GROUP, ch.shape[1]).max(axis=(1, 2)) / 127).astype(np.float32)
    step_rows = np.repeat(step, GROUP).astype(np.float64)
    q8 = np.clip(np.rint(qh / sq[:, None]), -127, 127)
    c8 = np.clip(np.rint(ch / step_rows[:, None]), -127, 127)
    e_rows = np.linalg.norm(ch - c8 * step_rows[:, None], axis=1)
    err = (e_rows.reshape(-1, GROUP).max(axis=1) * 1.001).astype(np.float32)
    e_q = np.linalg.norm(qh - q8 * sq[:, None], axis=1) * 1.001
    kq = (1.0001 + 3 * e_q).astype(np.float32)
    acc = q8 @ c8.T
    m = np.repeat(step, GROUP)[None, :] * sq[:, None]
    ek = np.repeat(err, GROUP)[None, :] * kq[:, None]
    R = (acc * m.astype(np.float64) + ek.astype(np.float64)).astype(np.float32)     # (fma: one rounding)
    R[:, REMOVED_ROW] = np.nan
    return acc, m, ek, R


def test_reference_accepts_the_emulated_kernel_and_rejects_a_shifted_slab(bf16_values):
    V = bf16_values
    mom = ref.emulate_slab_moments(V)
    w1, w2 = ref.check_moments(mom, V.astype(np.float64))
    assert 0 < w1 < 1 and 0 < w2 < 1
    for shifted in (np.roll(mom, 1, axis=1), np.roll(mom, 1, axis=0)):      # (a slab's slot; a query's)
        with pytest.raises(AssertionError):
            ref.check_moments(shifted, V.astype(np.float64))
    one = mom.copy()
    one[2, 17] = mom[2, 18]      # one slab of one query written from its neighbour
    with pytest.raises(AssertionError):
        ref.check_moments(one, V.astype(np.float64))
    half = V.copy()
    half[:, 64 * 9 + 32:64 * 10] = np.nan      # a row mask that drops half a slab
    with pytest.raises(AssertionError):
        ref.check_moments(ref.emulate_slab_moments(half), V.astype(np.float64))
    with_nan_rows = np.where(np.isnan(V), np.float32(0.5), V)      # a NaN image summed as a number
    with pytest.raises(AssertionError):
        ref.check_moments(ref.emulate_slab_moments(with_nan_rows), V.astype(np.float64))


def test_reference_rejects_the_int8_bound_term_left_in(i8_state):
    acc, m, ek, R = i8_state
    V, got_acc = ref.i8_terms(R, m, ek)
    ok = ~np.isnan(R)
    assert np.array_equal(got_acc[ok], acc[ok])
    good = np.where(ok, (acc.astype(np.float32) * m), np.float32(np.nan)).astype(np.float32)
    ref.check_moments(ref.emulate_slab_moments(good), V)
    with pytest.raises(AssertionError):      # the compared value, bound term and all, summed instead
        ref.check_moments(ref.emulate_slab_moments(R), V)
    with pytest.raises(AssertionError):      # a value that is no fl(acc m + ek): half an accumulator unit off
        ref.i8_terms((R.astype(np.float64) + 0.5 * m).astype(np.float32), m, ek)


@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_mirror_rejects_the_divisor_of_summed_rows(bf16_values, sample, metric):
    """two of the 16 384 rows are left out of the sums: dividing by 16 382 moves the model threshold by ~1e-4 of itself, a
    thousand float32 ulps"""
    Q, _ = sample
    mom = ref.emulate_slab_moments(bf16_values)
    counted = int((~np.isnan(bf16_values[0])).sum())
    assert counted == SAMPLE - 2
    zq = ref.zq_reference(58, N)
    nq = (Q.astype(np.float64) ** 2).sum(axis=1)
    for b in range(len(Q)):
        right = ref.model_threshold(metric, *(x[b] for x in ref.model_stats(mom, SAMPLE)), zq, 0.01, nq[b])
        wrong = ref.model_threshold(metric, *(x[b] for x in ref.model_stats(mom, counted)), zq, 0.01, nq[b])
        assert ref.ulps(right, wrong) > 2
    # ... and n in zq: the live rows instead of the size moves zq by more than 1e-9 as soon as one row is removed
    assert abs(ref.zq_reference(58, N) - ref.zq_reference(58, N - 1)) > 1e-9


def test_mirror_keeps_the_rigorous_threshold_for_a_model_that_is_no_number():
    """The rule "a model that is NaN or +inf leaves the rigorous threshold" as the MIRROR keeps it.  The device is not exercised:
    finite screen values cannot make its model NaN or infinite (and see below for what it would do with an infinite t)."""
    rig = np.float32(0.25)
    for bad in (np.float32(np.nan), np.float32(np.inf)):
        assert ref.published(rig, bad) == rig
    assert ref.published(rig, np.float32(0.2)) == rig and ref.published(rig, np.float32(0.3)) == np.float32(0.3)
    assert np.isnan(ref.model_threshold("cosine", np.nan, 0.1, 3.0, 0.01, 1.0))
    # an infinite t would NOT give an infinite model: float_below steps +inf down to the largest float.  It takes a sum of
    # squares that overflows float32; values of regular rows (norm <= 1e15) leave 16 384 of them four orders of magnitude short.
    assert ref.model_threshold("cosine", 0.0, np.inf, 3.0, 0.01, 1.0) == np.finfo(np.float32).max


def test_float_below_and_ulps():
    for x in (1.0, -1.0, 0.0, 1e-30, -3.5):
        y = ref.float_below(x)
        assert y < np.float32(x) and ref.ulps(y, np.float32(x)) == 1
    assert ref.float_below(-np.inf) == -np.inf and np.isnan(ref.float_below(np.nan))
    assert ref.ulps(np.float32(-np.inf), np.float32(-np.inf)) == 0 and ref.ulps(np.float32(1.0), np.float32(np.nan)) > 2
    assert K == 10
