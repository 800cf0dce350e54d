"""CPU: the numpy restatement of the search by examples and of Rocchio feedback (tests/examples_ref.py) against second
formulations -- a scalar Python loop for the combination, "the corpus with the listed rows deleted" for the strike --, and
the check that every feedback case of the GPU tests expects something else than the plain search."""

import math

import numpy as np
import pytest

import examples_ref as xr

NAN, INF = float("nan"), float("inf")


def small_corpus():
    rng = np.random.default_rng(41)
    C = rng.standard_normal((40, 13)).astype(np.float32)
    C[3] = 0.0                                   # zero row: no valid example
    C[4, 2] = NAN
    C[6] *= 1e20                                 # the squared norm overflows
    C[20] = C[21] = C[33] = C[8]                 # four exact copies
    live = np.ones(40, dtype=bool)
    live[[15, 21, 39]] = False                   # a removed ordinary row, a removed copy, the removed last row
    return C, live


def scalar_slot(oracle, C, q, pos, neg, alpha, beta, gamma, metric, row_offset, live):
    """one slot in plain Python floats (IEEE doubles): -> (q' as a list of float32, valid)"""
    nrm2 = oracle.row_nrm2(C)

    def scale(n2):
        return 1.0 / math.sqrt(float(n2)) if metric == "cosine" else 1.0

    def ok(n2):
        return math.isfinite(float(n2)) and float(n2) > 0.0

    def valid(ids):
        out = []
        for gid in ids:
            r = gid - row_offset
            if 0 <= r < len(C) and live[r] and ok(nrm2[r]):
                out.append(r)
        return out

    vp, vn = valid(pos), valid(neg)
    if q is not None:
        nq = oracle.row_nrm2(np.asarray(q, dtype=np.float32)[None, :])[0]
        if not ok(nq):
            return [0.0] * C.shape[1], 0
    elif not vp and not vn:
        return [0.0] * C.shape[1], 0
    out = []
    with np.errstate(all="ignore"):
        for i in range(C.shape[1]):
            acc = alpha * (scale(nq) * float(q[i])) if q is not None else 0.0
            for r in vp:
                acc = acc + (beta / float(len(vp))) * (scale(nrm2[r]) * float(C[r, i]))
            for r in vn:
                acc = acc - (gamma / float(len(vn))) * (scale(nrm2[r]) * float(C[r, i]))
            out.append(np.float32(acc))
    return out, 1


SLOTS = [  # (positives, negatives)
    ([1, 2, 8], [10]), ([8, 8, 20], []), ([3], [5]), ([3, 4, 6], [15]), ([-1, 7, -1], [9, -1]), ([40, 45, -3], [39]),
    ([], [11, 12]), ([21], []), ([2 ** 62, 0], [-2 ** 63]), ([30, 31], [30, 31]),
]


@pytest.mark.parametrize("metric", ["cosine", "ip"])
@pytest.mark.parametrize("with_base", [False, True])
def test_combine_equals_a_scalar_loop(oracle, metric, with_base):
    C, live = small_corpus()
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((len(SLOTS), C.shape[1])).astype(np.float32) if with_base else None
    if with_base:
        Q[1] = 0.0                               # invalid bases: zero, NaN, overflowing norm
        Q[2, 5] = NAN
        Q[4] *= 1e20
    pos, neg = [s[0] for s in SLOTS], [s[1] for s in SLOTS]
    for alpha, beta, gamma, off in ((1.0, 1.0, 1.0, 0), (0.0, 0.75, 0.25, 0), (0.3, 2.0, 0.0, 0), (1.0, 1.0, 1.0, 100)):
        gp = [[x + off for x in s] for s in pos]
        gn = [[x + off for x in s] for s in neg]
        vec, valid, stats = xr.combine(oracle, C, Q, gp, gn, alpha, beta, gamma, metric, off, live)
        n_bad_slots = 0
        for b in range(len(SLOTS)):
            want, ok = scalar_slot(oracle, C, None if Q is None else Q[b], gp[b], gn[b], alpha, beta, gamma, metric, off, live)
            assert valid[b] == ok
            n_bad_slots += 1 - ok
            assert vec[b].view(np.uint32).tolist() == np.array(want, dtype=np.float32).view(np.uint32).tolist(), (b, alpha)
        assert stats["skipped_slots"] == n_bad_slots
    # every position of the padded lists that is no live row with a finite positive norm is counted
    _, valid, stats = xr.combine(oracle, C, None, pos, neg, 1.0, 1.0, 1.0, metric, 0, live)
    nrm2 = oracle.row_nrm2(C)
    good = {r for r in range(len(C)) if live[r] and np.isfinite(nrm2[r]) and nrm2[r] > 0}
    assert good == set(range(40)) - {3, 4, 6, 15, 21, 39}
    listed = sum(len(s[0]) + len(s[1]) for s in SLOTS)
    assert stats["skipped"] == (3 + 2) * len(SLOTS) - listed + sum(x not in good for s in SLOTS for x in s[0] + s[1])
    assert valid.tolist() == [1, 1, 1, 0, 1, 0, 1, 0, 1, 1]
    # beta = gamma on the same row (or on a copy of it) cancels to exactly +0.0, and the slot stays valid
    vec, valid, _ = xr.combine(oracle, C, None, [[30], [8]], [[30], [20]], 1.0, 2.0, 2.0, metric, 0, live)
    assert not vec.view(np.uint32).any() and valid.tolist() == [1, 1]


@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_strike_equals_a_search_of_the_corpus_without_the_listed_rows(oracle, metric):
    """depth k + mp + mn is enough: the same lists come out of the oracle's top-k over the corpus with the listed (and the
    removed) rows deleted -- duplicates of a listed row stay, NaN rows keep their place"""
    C, live = small_corpus()
    pos, neg = [s[0] for s in SLOTS], [s[1] for s in SLOTS]
    for k in (1, 3, 10, 40):
        dist, rows, _ = xr.search_examples(oracle, C, None, pos, neg, 1.0, 1.0, 0.5, k, metric, 0, live)
        qp, valid, _ = xr.combine(oracle, C, None, pos, neg, 1.0, 1.0, 0.5, metric, 0, live)
        for b in range(len(SLOTS)):
            if not valid[b]:
                assert (rows[b] == -1).all() and np.isnan(dist[b]).all()
                continue
            left = np.array([r for r in range(len(C)) if live[r] and r not in pos[b] and r not in neg[b]])
            ds, rs = oracle.topk_search(np.ascontiguousarray(C[left]), qp[b:b + 1], k, metric=metric)
            want = np.where(rs[0] >= 0, left[np.maximum(rs[0], 0)], -1)
            xr.same_lists((dist[b:b + 1], rows[b:b + 1]), (ds, want[None, :]))
        # KEEP: the ordinary ranking of q' over the live rows
        dist, rows, _ = xr.search_examples(oracle, C, None, pos, neg, 1.0, 1.0, 0.5, k, metric, 0, live, keep=True)
        at = np.flatnonzero(valid)
        xr.same_lists((dist[at], rows[at]), xr.search_plain(oracle, C, qp[at], k, metric, 0, live))
    # a copy of a listed row stays in the answer, first (cosine: nothing is nearer than a copy)
    assert metric != "cosine" or xr.search_examples(oracle, C, None, [[8]], None, 1.0, 1.0, 1.0, 2, metric, 0, live)[1].tolist() == [[20, 33]]


@pytest.mark.parametrize("name", [c[0] for c in xr.FEEDBACK_CASES])
def test_feedback_cases_differ_from_the_plain_search(oracle, name):
    C, Q, metric, k, fb_k, alpha, beta = xr.feedback_case(name)
    dist, rows, stats, qp = xr.search_feedback(oracle, C, Q, k, fb_k, alpha, beta, metric)
    plain = xr.search_plain(oracle, C, Q, k, metric)
    assert (rows != plain[1]).any(axis=1).sum() >= 1, "the feedback moved no query's list: the case shows nothing"
    assert (rows >= 0).all() and stats == {"skipped": 0, "skipped_slots": 0}
    # by construction: the search at fb_k, then the search by examples with those rows and KEEP
    r1 = xr.search_plain(oracle, C, Q, fb_k, metric)[1]
    again = xr.search_examples(oracle, C, Q, r1, None, alpha, beta, 0.0, k, metric, keep=True)
    xr.same_lists(again, (dist, rows))
    assert again[2]["skipped"] == int((r1 < 0).sum())           # (the two-call form lists the padding: counted there)
