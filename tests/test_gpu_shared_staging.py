"""GPU: the host forms of every search family share ONE result staging on the handle (csrc/index.h: out_*_dev) and one query
staging.  Calls of different families and line widths, made one after the other on one handle, must each return exactly
what the same call returns on a fresh handle over the same corpus: nothing of an earlier call's lines, counts or widths
may show through.  Run in both orders; the range call takes its fallback (an inner search under an outer range call)."""

import ctypes

import numpy as np
import pytest

import range_ref

pytestmark = pytest.mark.gpu

N, D, B = 600, 32, 1030          # 1030 queries: two internal blocks in every host form
REMOVED, ZERO = 77, 123
M_RANGE, SLOTS = 7, 16           # option "range_slots": a count above 16 takes range search's fallback at 600 rows
GROUP_OFFSETS = [0, 3, 6, 9, 12]


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


@pytest.fixture(scope="module")
def case(pkg, oracle):
    rng = np.random.default_rng(20)
    C = rng.standard_normal((N, D)).astype(np.float32)
    C[ZERO] = 0.0                                    # NaN distances under cosine
    Q = rng.standard_normal((B, D)).astype(np.float32)
    live = np.ones(N, dtype=bool)
    live[REMOVED] = False
    ds, rs = range_ref.oracle_sorted(oracle, C, Q, "cosine")
    want = np.resize(np.array([M_RANGE, 0, 1, M_RANGE - 1, M_RANGE + 1, SLOTS + 5, 3]), B)   # some above max_results and above the slots
    radius, counts = range_ref.radius_admitting(ds, rs, want, live)
    assert (counts > SLOTS).any() and (counts > M_RANGE).any()
    slots = rng.integers(-2, N + 2, size=B).astype(np.int64)       # stored rows as queries: ids outside the index among them
    slots[:3] = [REMOVED, ZERO, 0]
    listed = rng.choice(N, size=100, replace=False).astype(np.int64)
    pools = rng.integers(-1, N, size=(40, 24)).astype(np.int64)    # mmr_select / score_subset: -1 padding and repeats

    def groups_without_count(idx):
        q, offs = np.ascontiguousarray(Q[:12]), np.asarray(GROUP_OFFSETS, dtype=np.int32)
        dist, rows = np.empty((4, 6), dtype=np.float64), np.empty((4, 6), dtype=np.int64)
        rc = idx._lib.mi355dr_search_groups(idx._h, q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                            offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 4, 6, 6,
                                            dist.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                            rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), None)
        assert rc == 0
        return dist, rows

    calls = [
        ("search", lambda idx: idx.search(Q, 5)),
        ("search_range", lambda idx: idx.search_range(Q, radius, M_RANGE)),
        ("search_mmr", lambda idx: idx.search_mmr(Q[:40], 3, 9, 0.5)),
        ("search_range_rows", lambda idx: idx.search_range_rows(slots, radius, 4)),
        ("search_groups", lambda idx: idx.search_groups(Q[:12], GROUP_OFFSETS, 6)),
        ("search_groups_no_count", groups_without_count),
        ("search_subset", lambda idx: idx.search_subset(Q[:40], 5, listed)),
        ("mmr_select", lambda idx: idx.mmr_select(Q[:40], 3, pools, 0.5)),
        ("score_subset", lambda idx: (idx.score_subset(Q[:40], pools),)),
        ("search_again", lambda idx: idx.search(Q, 5)),
    ]

    def make():
        idx = pkg.Mi355Index(D, "cosine")
        idx.add(C)
        idx.remove_rows([REMOVED])
        idx.set_option("range_slots", SLOTS)
        return idx

    fresh = {}
    for name, call in calls:                         # every reference from a handle that has made no other call
        with make() as idx:
            fresh[name] = call(idx)
    return make, calls, fresh


def assert_bit_equal(name, got, exp):
    assert len(got) == len(exp), name
    for g, e in zip(got, exp):
        assert g.shape == e.shape and g.dtype == e.dtype, name
        if g.dtype == np.float64:
            nan = np.isnan(e)
            assert np.array_equal(np.isnan(g), nan), f"{name}: NaN positions differ"
            assert np.array_equal(g[~nan].view(np.uint64), e[~nan].view(np.uint64)), f"{name}: distance bits differ"
        else:
            assert np.array_equal(g, e), f"{name}: rows or counts differ"


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_families_sharing_one_staging_return_what_a_fresh_handle_returns(case, order):
    make, calls, fresh = case
    with make() as idx:
        for name, call in (calls if order == "forward" else calls[::-1]):
            assert_bit_equal(name, call(idx), fresh[name])
        assert idx.stat("range_fallback_queries") > 0
