"""Shared by the tests of the speculative one-chunk pass: test_gpu_speculative.py, test_gpu_spec_threshold.py,
test_gpu_spec_callers.py."""

import numpy as np

SPEC_STATS = ("spec_passes", "passes", "chunks", "spec_miss_queries", "spec_overflow_queries", "retry_queries", "fallback_queries")


def same(got, want):
    (dist, rows), (rd, rr) = got, want
    assert np.array_equal(rows, rr)
    assert np.array_equal(np.isnan(dist), np.isnan(rd))  # NaN payload/sign is not part of the contract
    ok = ~np.isnan(rd)
    assert np.array_equal(dist[ok].view(np.uint64), rd[ok].view(np.uint64))


def arm(idx, rows=None):
    """lower `spec_min_rows` to the index's size (or `rows`) and make every pass that is not speculative recognisable"""
    idx.set_option("spec_min_rows", len(idx) if rows is None else rows)
    # four samples of rows are ONE step of the default ladder as well (ratio 4): chunk ratios of at most 2 make every pass
    # that is not speculative recognisable by its two chunks.  A speculative pass has no ratio to grow by.
    idx.set_option("chunk_growth", 1)
    return idx


def index(pkg, C, metric="cosine"):
    idx = pkg.Mi355Index(C.shape[1], metric)
    idx.add(C)
    return arm(idx, len(C))


PLANTED_N, PLANTED_D, PLANTED_PAIRS = 65536, 64, 8


def planted_corpus():
    """(C, Q): the best rows of the first 8 queries inside the sample (rows 100 + 37 i), each with an exact duplicate at the far
    end (row N - 1 - i; a tie: the lower row first); zero rows; a row the int8 shadow cannot hold; a zero query and a NaN query"""
    N = PLANTED_N
    rng = np.random.default_rng(21)
    C = rng.standard_normal((N, PLANTED_D)).astype(np.float32)
    Q = rng.standard_normal((48, PLANTED_D)).astype(np.float32)
    for i in range(PLANTED_PAIRS):
        C[100 + 37 * i] = Q[i] * np.float32(1.5)
        C[N - 1 - i] = C[100 + 37 * i]
    C[[5, 20000, N - 20]] = 0.0
    C[30000] = 0.01 * C[30000]
    C[30000, 3] = 9.0   # (one dominant component: outside the int8 shadow)
    Q[20] = 0.0
    Q[21, 7] = np.nan
    return C, Q


# ---- the corpus of the threshold tests (test_gpu_spec_threshold.py; its checks are shown to fail in test_spec_model_ref.py) ----
THR_N, THR_K = 65536, 10
SAMPLE, SLICE, GROUP = 16384, 2048, 32
ZERO_ROW, LOOSE_ROW, REMOVED_ROW, UPDATED_ROW = 5, 3000, 7001, 9002   # all inside the sample
ZERO_Q, NAN_Q = 20, 21
B_ALL = 130


def threshold_case(d, seed):
    """(C, the updated row's new vector, Q) of test_gpu_spec_threshold.py: Gaussian rows; a zero row, a row outside the int8
    shadow, and (for the test to remove / update) two more inside the sample; a zero query and a NaN query"""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((THR_N, d)).astype(np.float32)
    C[ZERO_ROW] = 0.0
    C[LOOSE_ROW] = 0.01 * C[LOOSE_ROW]
    C[LOOSE_ROW, 3] = 9.0   # (one dominant component: outside the int8 shadow)
    new = (3.0 * rng.standard_normal(d)).astype(np.float32)
    Q = rng.standard_normal((B_ALL, d)).astype(np.float32)
    Q[ZERO_Q] = 0.0
    Q[NAN_Q, 7] = np.nan
    return C, new, Q


def counters(idx):
    return {s: idx.stat(s) for s in SPEC_STATS}
