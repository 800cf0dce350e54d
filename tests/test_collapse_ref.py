"""CPU: tests/collapse_ref.py, the reference of the source cap -- the plain walk against a second, independent formulation
(rank within the key by one stable sort) over seeded random lists and over every shared input, and on cases worked by hand."""

import numpy as np
import pytest

import collapse_ref as cr


def test_hand_cases():
    for name, vals, ids, keys, cap, k_out, want_ids, want_count in cr.hand_cases():
        got = cr.collapse(vals, ids, keys, cap, k_out)
        assert got.ids[0].tolist() == want_ids, name
        assert int(got.count[0]) == want_count, name
        assert int(got.entries[0]) == int((ids[0] >= 0).sum()), name
        kept = got.ids[0] >= 0
        assert np.isnan(got.vals[0][~kept]).all() and (got.pos[0][~kept] == -1).all() and (got.keys[0][~kept] == -1).all(), name
        # a kept entry is the input's entry at its position, bit for bit
        p = got.pos[0][kept]
        assert np.array_equal(ids[0][p], got.ids[0][kept]) and np.all(np.diff(p) > 0), name
        assert np.array_equal(vals.view(np.uint64)[0][p], got.vals.view(np.uint64)[0][kept]), name


def test_values_keep_their_bits():
    vals = np.array([[0.0, -0.0, np.inf, -np.inf, np.nan, 1.5]])
    vals.view(np.uint64)[0, 4] = np.uint64(0x7FF80000DEADBEEF)
    ids = np.arange(6, dtype=np.int64)[None, :]
    got = cr.collapse(vals, ids, None, 1, 8)
    assert np.array_equal(got.vals.view(np.uint64)[0, :6], vals.view(np.uint64)[0])
    assert (got.vals.view(np.uint64)[0, 6:] == cr.NAN_BITS).all() and got.count[0] == 6


@pytest.mark.parametrize("seed", range(6))
def test_walk_equals_rank_formulation_on_random_lists(seed):
    rng = np.random.default_rng(seed)
    for _ in range(40):
        B, w = int(rng.integers(1, 4)), int(rng.integers(1, 200))
        n_ids = int(rng.integers(1, 2 * w + 2))
        ids = rng.integers(-2, n_ids + 5, size=(B, w)).astype(np.int64)
        keys = rng.integers(-3, max(2, w // 4), size=n_ids).astype(np.int64)
        keys[rng.random(n_ids) < 0.1] = cr.INT64_MAX
        vals = rng.standard_normal((B, w))
        vals[rng.random((B, w)) < 0.05] = np.nan
        cap, k_out = int(rng.integers(1, 5)), int(rng.integers(1, w + 4))
        table = None if rng.random() < 0.1 else keys
        cr.same(cr.collapse_by_rank(vals, ids, table, cap, k_out), cr.collapse(vals, ids, table, cap, k_out), f"seed {seed}")


def test_walk_equals_rank_formulation_on_the_shared_inputs():
    inputs = cr.all_inputs()
    assert len(inputs) > 150
    widths = set()
    for name, vals, ids, keys, cap in inputs:
        w = ids.shape[1]
        widths.add(w)
        exp = cr.collapse(vals, ids, keys, cap, w)
        cr.same(cr.collapse_by_rank(vals, ids, keys, cap, w), exp, name)
        assert (exp.count <= exp.entries).all() and (exp.entries <= w).all(), name
    assert widths == {1, 63, 64, 65, 257, 1024, 1025, 4096}
    # the inputs are not vacuous: somewhere the cap strikes entries, somewhere it strikes none, somewhere nothing is an entry
    struck = [int((cr.collapse(v, i, k, c, i.shape[1]).entries - cr.collapse(v, i, k, c, i.shape[1]).count).sum())
              for _, v, i, k, c in inputs[::7]]
    assert any(s > 0 for s in struck) and any(s == 0 for s in struck)
    assert any((i < 0).all() for _, _, i, _, _ in inputs)


def test_search_result_states():
    dist = np.arange(8, dtype=np.float64)[None, :].repeat(3, axis=0)
    rows = np.array([[0, 1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 7], [0, 1, 2, -1, -1, -1, -1, -1]], dtype=np.int64)
    keys = np.array([1, 1, 1, 1, 1, 1, 1, 2], dtype=np.int64)
    d, r, k, count, state = cr.search_result(dist, rows, keys, 1, 2, 8)
    assert r.tolist() == [[0, 7], [0, 7], [0, -1]] and count.tolist() == [2, 2, 1] and state.tolist() == [0, 0, 0]
    d, r, k, count, state = cr.search_result(dist, rows, keys, 1, 2, 4)   # cut at 4: lines 0 and 1 are truncated, line 2 ended
    assert r.tolist() == [[0, -1], [0, -1], [0, -1]] and count.tolist() == [1, 1, 1] and state.tolist() == [1, 1, 0]
