"""CPU: the reference of "MaxSim explained" (tests/maxsim_align_ref.py) against a second, scalar formulation, against the
oracle's MaxSim distance, and on hand-made documents for the tie, padding, NaN and clamp rules."""

import math

import numpy as np
import pytest

import maxsim_align_ref as ref

F32 = np.float32


def _unit(rng, n, d):
    v = rng.standard_normal((n, d)).astype(F32)
    return v / np.linalg.norm(v, axis=1, keepdims=True).astype(F32)


@pytest.fixture(scope="module")
def small(oracle):
    """five documents (one empty), two queries (7 and 3 vectors), d = 20; candidates with an unknown id and -1 padding"""
    rng = np.random.default_rng(11)
    d, lens = 20, [5, 0, 33, 1, 12]
    store = ref.RefStore(d)
    docs = [_unit(rng, t, d) for t in lens]
    store.add_multivec(np.concatenate(docs), np.concatenate([[0], np.cumsum(lens)]))
    q = _unit(rng, 10, d)
    qoff = np.array([0, 7, 10], dtype=np.int32)
    ids = np.array([[0, 1, 2, 3, 4, 9, -1], [4, 4, -1, 2, 0, 1, -7]], dtype=np.int64)
    return store, docs, q, qoff, ids, store.maxsim_align(q, qoff, ids)


def test_reference_equals_a_scalar_formulation(small, oracle):
    """A second statement of the rule, element by element in Python floats: C's fmaf chain via the oracle's dot, math-level max
    and first index."""
    store, docs, q, qoff, ids, al = small
    for b in range(2):
        for p in range(ids.shape[1]):
            i = int(ids[b, p])
            live = 0 <= i < len(docs) and docs[i].shape[0] > 0
            for g in range(qoff[b], qoff[b + 1]):
                if not live:
                    assert math.isnan(al.values[g, p]) and al.tokens[g, p] == -1
                    continue
                best, arg = -math.inf, -1
                for j in range(docs[i].shape[0]):
                    v = oracle.dot(q[g], docs[i][j])
                    if v > best:   # strictly greater: the lowest index keeps a tie
                        best, arg = v, j
                assert F32(best).view(np.uint32) == al.values[g, p].view(np.uint32) and arg == al.tokens[g, p]
            assert math.isnan(al.dist[b, p]) == (not live)


def test_ordered_sum_of_the_values_is_the_oracle_distance(small, oracle):
    store, docs, q, qoff, ids, al = small
    for b in range(2):
        qb = q[qoff[b]:qoff[b + 1]]
        for p in range(ids.shape[1]):
            i = int(ids[b, p])
            if 0 <= i < len(docs) and docs[i].shape[0] > 0:
                want = F32(oracle.maxsim_distance(docs[i], qb))
                acc = F32(0.0)
                for g in range(qoff[b], qoff[b + 1]):
                    acc = F32(acc + F32(-al.values[g, p]))
                assert acc.view(np.uint32) == want.view(np.uint32) == al.dist[b, p].view(np.uint32)


def test_maps_hold_the_alignment(small, oracle):
    store, docs, q, qoff, ids, al = small
    maps = store.maxsim_map(q, qoff, [0, 1, 0, 1], [2, 2, 1, 77])
    assert [m.shape for m in maps] == [(7, 33), (3, 33), (7, 0), (3, 0)]
    assert np.array_equal(maps[0].max(axis=1).view(np.uint32), al.values[0:7, 2].view(np.uint32))
    assert np.array_equal(maps[0].argmax(axis=1), al.tokens[0:7, 2])
    assert np.array_equal(maps[1].argmax(axis=1), al.tokens[7:10, 3])
    assert np.array_equal(store.multivec_token_counts([0, 1, 2, 5, -1]), [5, 0, 33, -1, -1])


def test_ties_nan_and_clamp_on_hand_made_documents(oracle):
    d = 8
    e = np.eye(d, dtype=F32)
    nan = np.full(d, np.nan, dtype=F32)
    store = ref.RefStore(d)
    docs = [np.stack([e[1], e[0], e[2], e[0]]),        # 0: e0 twice, at 1 and 3 -> 1
            np.stack([nan, e[0], nan]),                # 1: NaN tokens are ignored -> 1
            np.stack([nan, nan]),                      # 2: nothing but NaN -> -inf / -1
            np.stack([-e[0], -2 * e[0], -e[0]])]       # 3: all dots negative: best at 0 (tie with 2)
    store.add_multivec(np.concatenate(docs), np.cumsum([0] + [t.shape[0] for t in docs]))
    q = np.stack([e[0], e[0] + e[2]])
    al = store.maxsim_align(q, [0, 2], [[0, 1, 2, 3]])
    assert al.tokens.tolist() == [[1, 1, -1, 0], [1, 1, -1, 0]]
    assert al.values[:, 0].tolist() == [1.0, 1.0] and al.values[:, 1].tolist() == [1.0, 1.0]
    assert np.all(np.isneginf(al.values[:, 2])) and np.isposinf(al.dist[0, 2])
    assert al.values[:, 3].tolist() == [-1.0, -1.0] and al.dist[0, 3] == 2.0
    cl = store.maxsim_align(q, [0, 2], [[0, 1, 2, 3]], clamp0=True)
    assert cl.tokens.tolist() == al.tokens.tolist()                       # the token is the unclamped argmax
    assert cl.values[:, 3].tolist() == [0.0, 0.0] and cl.values[:, 2].tolist() == [0.0, 0.0]
    assert cl.dist[0].tolist() == [-2.0, -2.0, 0.0, 0.0]
    # a query without vectors: no value rows, a NaN distance row
    al0 = store.maxsim_align(q, [0, 0, 2], [[0, 1], [0, 1]])
    assert al0.values.shape == (2, 2) and np.all(np.isnan(al0.dist[0])) and not np.any(np.isnan(al0.dist[1]))
