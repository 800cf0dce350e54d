"""The Guided Query Refinement kernels (csrc/k_gqr.h) at the shapes tests/test_gpu_gqr.py never reaches, against the CPU
oracle (oracle/gqr_ref.py, numpy float64): full pools of 2048 candidates (eight trips of every strided loop), the second
trip of exactly one thread, d < 64 and d = 1, all-padding pools, the general MFMA form at dpad % 16 == 8 and above 128,
three and seven query chunks, ragged chunks inside a longer nq_pad, np.argmax's first-maximum rule under exact ties, the
LDS ceiling and the argument limits.  Every live entry is compared; NaN must sit exactly at the padding."""

from functools import lru_cache

import numpy as np
import pytest

# float64 on both sides; the only differences are summation order and exp's last bit, compounded over <= 40 steps
ATOL = 1e-10
PARAMS = [(25, 0.1, 1.0, 0.5), (3, 0.5, 0.05, 1.0), (40, 1.5, 0.3, 0.25)]  # the three sets of tests/golden/gqr_golden.npz
OFFSET = 2**33  # a shard's row_offset beyond int32

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def _assert_close(got, exp, what=""):
    assert np.array_equal(np.isnan(got), np.isnan(exp)), what  # NaN exactly at the padding
    live = ~np.isnan(exp)
    err = float(np.abs(got[live] - exp[live]).max()) if live.any() else 0.0
    print(f"{what}: max |gpu - oracle| = {err:.3e} over {int(live.sum())} live entries")
    assert err <= ATOL, what


def _cut(pools, comp, b, m):
    """query b keeps a live prefix of m candidates; the rest is -1 padding"""
    pools[b, m:] = -1
    comp[b, m:] = 0
    if m:
        comp[b] /= comp[b].sum()


# ---- single-vector form ------------------------------------------------------------------------------------------------
# (P, d, queries, parameter sets): pools are drawn without replacement from an index of P + 50 rows
SINGLE = {
    "P2048_d768": (2048, 768, 2, PARAMS[:1]),  # 8 trips of every strided loop, 70 KiB of LDS (above the 64 KiB default)
    "P2048_d64": (2048, 64, 3, PARAMS),        # full pool, one lane-trip per dot
    "P257_d7": (257, 7, 4, PARAMS),            # second trip of exactly one thread; d < 64; ragged and all-padding pools
    "P256_d100": (256, 100, 3, PARAMS),        # exactly one trip; d not a multiple of 64
    "P300_d1": (300, 1, 3, PARAMS),            # every cosine is +-1
}


@lru_cache(maxsize=None)
def _single_case(name):
    P, d, B, _ = SINGLE[name]
    rng = np.random.default_rng(1000 + P + d)
    n = P + 50
    C = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((B, d)).astype(np.float32).astype(np.float64)
    pools = np.stack([rng.choice(n, size=P, replace=False) for _ in range(B)]).astype(np.int64)
    comp = rng.dirichlet(np.ones(P), size=B)
    if name == "P257_d7":
        _cut(pools, comp, 1, 255)
        _cut(pools, comp, 2, 0)  # all padding, between two live neighbours
    return C, Q, pools, comp


def _single_expected(C, Q, pools, comp, prm):
    from oracle import gqr_ref

    out = np.full(pools.shape, np.nan)
    Cd = C.astype(np.float64)
    for b in range(pools.shape[0]):
        m = int((pools[b] >= 0).sum())
        if m:
            out[b, :m] = gqr_ref.refine_single(Q[b], Cd[pools[b, :m]], comp[b, :m], *prm)
    return out


@gpu
@pytest.mark.parametrize("name,s", [(nm, s) for nm, c in SINGLE.items() for s in range(len(c[3]))])
def test_single_vector_form_matches_oracle(pkg, name, s):
    C, Q, pools, comp = _single_case(name)
    prm = SINGLE[name][3][s]
    with pkg.Mi355Index(C.shape[1]) as idx:
        idx.add(C)
        got = idx.gqr_refine(Q, pools, comp, *prm)
    _assert_close(got, _single_expected(C, Q, pools, comp, prm), f"single {name} {prm}")
    if name == "P257_d7":
        assert np.isnan(got[2]).all() and not np.isnan(got[1, :255]).any() and np.isnan(got[1, 255:]).all()


@gpu
def test_single_vector_form_row_offset_beyond_int32(pkg):
    """global ids of a shard (row_offset = 2^33): bit-identical to the unshifted call, ragged and all-padding pools included"""
    C, Q, pools, comp = _single_case("P257_d7")
    with pkg.Mi355Index(C.shape[1]) as idx:
        idx.add(C)
        got = idx.gqr_refine(Q, pools, comp, *PARAMS[0])
        idx.set_option("row_offset", OFFSET)
        shifted = idx.gqr_refine(Q, np.where(pools >= 0, pools + OFFSET, pools), comp, *PARAMS[0])
        with pytest.raises(pkg.NativeError, match="not a row"):
            idx.gqr_refine(Q, pools, comp, *PARAMS[0])  # local ids are no rows of this shard any more
    assert np.array_equal(got, shifted, equal_nan=True)
    assert np.array_equal(np.isnan(got), pools < 0)


# ---- score form ----------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _score_case(P):
    rng = np.random.default_rng(2000 + P)
    counts = np.array([P, 0, 1, 257], dtype=np.int32)
    z = rng.standard_normal((4, P)).astype(np.float32).astype(np.float64)
    comp = rng.dirichlet(np.ones(P), size=4)
    for b, m in enumerate(counts):
        comp[b, m:] = 0
        if m:
            comp[b] /= comp[b].sum()
    return z, counts, comp


def _score_expected(z, counts, comp, prm):
    from oracle import gqr_ref

    out = np.full(z.shape, np.nan)
    for b, m in enumerate(counts):
        out[b, :m] = gqr_ref.refine_scores(z[b, :m], comp[b, :m], *prm)
    return out


@gpu
@pytest.mark.parametrize("P", [2048, 300])
@pytest.mark.parametrize("s", range(3))
def test_score_form_matches_oracle(pkg, P, s):
    """counts[b] == P, 0, 1 and 257 in one call"""
    z, counts, comp = _score_case(P)
    with pkg.Mi355Index(8) as idx:
        got = idx.gqr_refine_scores(z, counts, comp, *PARAMS[s])
    _assert_close(got, _score_expected(z, counts, comp, PARAMS[s]), f"scores P={P} {PARAMS[s]}")
    assert np.isnan(got[1]).all() and np.isnan(got[2, 1:]).all() and not np.isnan(got[0]).any()


@gpu
def test_score_form_temperature_below_the_floor(pkg):
    """temperature 1e-9 is floored at 1e-8 on both sides; one step is about 1e8 large, so the comparison is relative"""
    z, counts, comp = _score_case(300)
    prm = (1, 0.1, 1e-9, 0.5)
    with pkg.Mi355Index(8) as idx:
        got = idx.gqr_refine_scores(z, counts, comp, *prm)
        floored = idx.gqr_refine_scores(z, counts, comp, 1, 0.1, 1e-8, 0.5)
    exp = _score_expected(z, counts, comp, prm)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    live = ~np.isnan(exp)
    rel = np.abs(got[live] - exp[live]) / np.abs(exp[live])
    print(f"T = 1e-9: max relative difference {rel.max():.3e}, largest |score| {np.abs(exp[live]).max():.3e}")
    assert np.abs(exp[live]).max() > 1e3  # the step is as large as the case is meant to be
    assert (np.abs(got[live] - exp[live]) <= 1e-12 * np.abs(exp[live])).all()
    assert np.array_equal(got, floored, equal_nan=True)


@gpu
def test_score_form_infinite_score_takes_the_uniform_branch(pkg):
    """+inf among the primary scores: the softmax normaliser is not finite, both sides fall back to 1/n each"""
    from oracle import gqr_ref

    z, counts, comp = (a.copy() for a in _score_case(300))
    z[0, 5] = np.inf
    with pkg.Mi355Index(8) as idx:
        got = idx.gqr_refine_scores(z, counts, comp, *PARAMS[0])
    with np.errstate(invalid="ignore"):
        exp = _score_expected(z, counts, comp, PARAMS[0])
        uniform = z[0] - PARAMS[0][0] * PARAMS[0][1] * gqr_ref.logit_grad(np.zeros(300), comp[0], 1.0, 0.5)
    assert got[0, 5] == np.inf and exp[0, 5] == np.inf
    finite = np.ones(z.shape, bool)
    finite[0, 5] = False
    _assert_close(np.where(finite, got, np.nan), np.where(finite, exp, np.nan), "scores with +inf")
    assert np.abs(np.delete(exp[0], 5) - np.delete(uniform, 5)).max() <= ATOL  # (the oracle took the uniform branch: p = 1/n every step)


# ---- multi-vector form ---------------------------------------------------------------------------------------------------
def _unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _ragged_docs(rng, n_docs, d):
    """documents of 1..70 normalised tokens; the first five have 1, 31, 32, 33 and 64 (around the store's 32-row blocks)"""
    lens = rng.integers(1, 71, size=n_docs)
    lens[:5] = (1, 31, 32, 33, 64)
    return _unit_rows(rng, int(lens.sum()), d), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _pools(rng, n_docs, B, P):
    """pools without replacement; the store's last document is never a candidate, query 0 holds documents 0..4"""
    pools = np.stack([rng.choice(n_docs - 1, size=P, replace=False) for _ in range(B)]).astype(np.int64)
    pools[0] = rng.permutation(np.concatenate([np.arange(5), 5 + rng.choice(n_docs - 6, size=P - 5, replace=False)]))
    return pools


# (d, query lengths of one call, P, parameter sets)
MULTI = {
    "d24_q48_5_17": (24, (48, 5, 17), 300, PARAMS),   # dpad 24: half-empty last K-step; three chunks; ragged chunks in nq_pad 48
    "d20_q1_16_33": (20, (1, 16, 33), 600, PARAMS),   # dpad 24 with four zero-padded columns behind the permutation
    "d8_q1_1": (8, (1, 1), 2048, PARAMS),             # full pool; the only K-step is half empty
    "d200_q33_2": (200, (33, 2), 64, PARAMS),         # dpad > 128 in the general form, 76 KiB of LDS
    "d128_q100_32": (128, (100, 32), 40, PARAMS),     # seven chunks in the unrolled form
    "d128_q144_ceiling": (128, (144,), 585, PARAMS[1:2]),  # 163 832 bytes of LDS: eight under the 160 KiB ceiling
}


@lru_cache(maxsize=None)
def _multi_case(name):
    d, q_lens, P, _ = MULTI[name]
    rng = np.random.default_rng(3000 + d + P)
    n_docs = P + 51
    tok, off = _ragged_docs(rng, n_docs, d)
    qtok = _unit_rows(rng, sum(q_lens), d).astype(np.float64)
    qoff = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    pools = _pools(rng, n_docs, len(q_lens), P)
    comp = rng.dirichlet(np.ones(P), size=len(q_lens))
    if name == "d24_q48_5_17":
        _cut(pools, comp, 1, 290)
    return tok, off, qtok, qoff, pools, comp


def _multi_expected(tok, off, qtok, qoff, pools, comp, prm):
    from oracle import gqr_ref

    out = np.full(pools.shape, np.nan)
    tokd = tok.astype(np.float64)
    for b in range(pools.shape[0]):
        m = int((pools[b] >= 0).sum())
        docs = [tokd[off[i]:off[i + 1]] for i in pools[b, :m]]
        out[b, :m] = gqr_ref.refine_multi(qtok[qoff[b]:qoff[b + 1]], docs, comp[b, :m], *prm)
    return out


@gpu
@pytest.mark.parametrize("name,s", [(nm, s) for nm, c in MULTI.items() for s in range(len(c[3]))])
def test_multi_vector_form_matches_oracle(pkg, name, s):
    tok, off, qtok, qoff, pools, comp = _multi_case(name)
    prm = MULTI[name][3][s]
    with pkg.Mi355Index(tok.shape[1]) as idx:
        idx.add_multivec(tok, off)
        got = idx.gqr_refine_maxsim(qtok, qoff, pools, comp, *prm)
    _assert_close(got, _multi_expected(tok, off, qtok, qoff, pools, comp, prm), f"multi {name} {prm}")


@gpu
def test_multi_vector_form_row_offset_beyond_int32(pkg):
    tok, off, qtok, qoff, pools, comp = _multi_case("d24_q48_5_17")
    with pkg.Mi355Index(tok.shape[1]) as idx:
        idx.add_multivec(tok, off)
        got = idx.gqr_refine_maxsim(qtok, qoff, pools, comp, *PARAMS[0])
        idx.set_option("row_offset", OFFSET)
        shifted = idx.gqr_refine_maxsim(qtok, qoff, np.where(pools >= 0, pools + OFFSET, pools), comp, *PARAMS[0])
        with pytest.raises(pkg.NativeError, match="not a row"):
            idx.gqr_refine_maxsim(qtok, qoff, pools, comp, *PARAMS[0])
    assert np.array_equal(got, shifted, equal_nan=True)
    assert np.array_equal(np.isnan(got), pools < 0)


# ---- the first-maximum rule ------------------------------------------------------------------------------------------------
# Two distinct tokens A and B of one document tie exactly for query vector 0 at step 0: the query vector and both tokens
# hold small integers, so their dot products (5 and 5) are exact in any summation order, on the f64 matrix pipe and in
# BLAS alike.  A and B differ only in column 2, where the query vector is 0 -- A[2] = 3, B[2] = 1 -- so whichever of them
# the argmax names pulls that column by another amount in the first gradient step, and every later score depends on it.
# The rest of the document has zeros in the two columns the query vector uses (dot product exactly 0), all other
# documents and query vectors are Gaussian: no second tie exists, and after step 0 not even this one.
# (first position, second position, document length): where the tying pair sits in the store's 32-row blocks
PLACEMENTS = {
    "same_tile": (3, 9, 20),               # one 16-token tile, different lanes
    "tile_a_tile_b_same_lane": (5, 21, 30),  # the two tiles of one block, met by one lane in turn
    "tile_a_tile_b": (5, 22, 30),
    "block0_block1_same_lane": (7, 39, 50),
    "block0_block1": (7, 40, 50),
    "first_and_last_of_33": (0, 32, 33),   # the last token is repeated 31 times behind itself as block padding
}
TIE_D, TIE_NQ, TIE_P = 8, 4, 8


@lru_cache(maxsize=None)
def _tie_case(place, a_first):
    """(docs of one pool -- document 0 holds the pair --, query matrix, complementary distribution)"""
    first, second, length = PLACEMENTS[place]
    rng = np.random.default_rng(4000 + 10 * list(PLACEMENTS).index(place))  # the same draw for both orders
    A = np.array([2, 1, 3, 0, 0, 0, 0, 0], dtype=np.float32)
    B = np.array([2, 1, 1, 0, 0, 0, 0, 0], dtype=np.float32)
    special = np.zeros((length, TIE_D), dtype=np.float32)
    special[:, 2:] = _unit_rows(rng, length, TIE_D - 2)
    special[first], special[second] = (A, B) if a_first else (B, A)
    docs = [special] + [_unit_rows(rng, int(t), TIE_D) for t in rng.integers(1, 71, size=TIE_P - 1)]
    Q = _unit_rows(rng, TIE_NQ, TIE_D).astype(np.float64)
    Q[0] = (2, 1, 0, 0, 0, 0, 0, 0)
    comp = rng.dirichlet(np.ones(TIE_P))
    return docs, Q, comp


@pytest.mark.parametrize("place", list(PLACEMENTS))
@pytest.mark.parametrize("s", range(3))
def test_oracle_first_maximum_precondition(place, s):
    """(CPU) which of the two tying tokens comes first changes refine_multi's result by far more than the GPU test's
    tolerance: without this the GPU test could not tell the first maximum from the last."""
    from oracle import gqr_ref

    res = []
    for a_first in (True, False):
        docs, Q, comp = _tie_case(place, a_first)
        first, second, _ = PLACEMENTS[place]
        dots = docs[0].astype(np.float64) @ Q[0]
        assert dots[first] == dots[second] == 5.0 and np.delete(dots, [first, second]).max() == 0.0
        assert int(np.argmax(dots)) == first
        res.append(gqr_ref.refine_multi(Q, docs, comp, *PARAMS[s]))
    assert np.abs(res[0] - res[1]).max() > 1e-6


@gpu
@pytest.mark.parametrize("s", range(3))
def test_multi_vector_form_keeps_the_first_maximum(pkg, s):
    """every placement of the tying pair, in both orders, as the queries of one call"""
    from oracle import gqr_ref

    cases = [_tie_case(place, a_first) for place in PLACEMENTS for a_first in (True, False)]
    # (one more document behind the last candidate: a kernel that reads a few columns past a row stays inside the store)
    all_docs = [t for docs, _, _ in cases for t in docs] + [np.ones((1, TIE_D), dtype=np.float32)]
    off = np.concatenate([[0], np.cumsum([t.shape[0] for t in all_docs])]).astype(np.int64)
    pools = np.arange(len(cases) * TIE_P, dtype=np.int64).reshape(len(cases), TIE_P)
    qtok = np.concatenate([Q for _, Q, _ in cases])
    qoff = (np.arange(len(cases) + 1) * TIE_NQ).astype(np.int32)
    comp = np.stack([c for _, _, c in cases])
    with pkg.Mi355Index(TIE_D) as idx:
        idx.add_multivec(np.concatenate(all_docs), off)
        got = idx.gqr_refine_maxsim(qtok, qoff, pools, comp, *PARAMS[s])
    exp = np.stack([gqr_ref.refine_multi(Q, docs, c, *PARAMS[s]) for docs, Q, c in cases])
    names = [f"{place}/{'AB' if a_first else 'BA'}" for place in PLACEMENTS for a_first in (True, False)]
    err = np.abs(got - exp).max(axis=1)
    print({n: f"{e:.2e}" for n, e in zip(names, err)})
    assert [n for n, e in zip(names, err) if not e <= ATOL] == []


@gpu
@pytest.mark.parametrize("d", [24, 128])
def test_all_zero_query_vector_takes_token_zero(pkg, d):
    """an all-zero query vector scores 0 against every token of every document: token 0 must carry the subgradient (the
    documents of 1, 31, 32, 33 and 64 tokens are in the pool)"""
    rng = np.random.default_rng(4500 + d)
    n_docs, P = 60, 40
    tok, off = _ragged_docs(rng, n_docs, d)
    qtok = _unit_rows(rng, 3 + 18, d).astype(np.float64)
    qtok[1] = 0.0   # query 0: the middle one of three vectors
    qtok[20] = 0.0  # query 1: the last of 18, in the second chunk
    qoff = np.array([0, 3, 21], dtype=np.int32)
    pools = _pools(rng, n_docs, 2, P)
    comp = rng.dirichlet(np.ones(P), size=2)
    with pkg.Mi355Index(d) as idx:
        idx.add_multivec(tok, off)
        for prm in PARAMS:
            got = idx.gqr_refine_maxsim(qtok, qoff, pools, comp, *prm)
            _assert_close(got, _multi_expected(tok, off, qtok, qoff, pools, comp, prm), f"zero query vector d={d} {prm}")


# ---- limits: error returns, not launches ---------------------------------------------------------------------------------
@gpu
def test_pool_limit_of_2048_candidates(pkg):
    P = 2049
    comp = np.full((1, P), 1.0 / P)
    pool = np.zeros((1, P), dtype=np.int64)
    with pkg.Mi355Index(8) as idx:
        idx.add(np.eye(8, dtype=np.float32))
        with pytest.raises(pkg.NativeError, match="2048"):
            idx.gqr_refine(np.ones((1, 8)), pool, comp, *PARAMS[0])
        with pytest.raises(pkg.NativeError, match="2048"):
            idx.gqr_refine_scores(np.zeros((1, P)), [P], comp, *PARAMS[0])
        with pytest.raises(pkg.NativeError, match="2048"):
            idx.gqr_refine_maxsim(np.ones((2, 8)), [0, 2], pool, comp, *PARAMS[0])


@gpu
def test_multi_vector_form_refusals(pkg):
    rng = np.random.default_rng(4600)
    d = 128
    tok, off = _ragged_docs(rng, 12, d)
    comp = np.full((1, 4), 0.25)
    pool = np.array([[0, 1, 2, 3]], dtype=np.int64)
    with pkg.Mi355Index(d) as idx:
        idx.add_multivec(tok, off)
        q = _unit_rows(rng, 160, d).astype(np.float64)
        # 160 query vectors: the query matrix alone is 160 * 130 doubles, above 160 KiB of LDS whatever the pool
        with pytest.raises(pkg.NativeError, match="too large"):
            idx.gqr_refine_maxsim(q, [0, 160], pool, comp, *PARAMS[0])
        assert idx.gqr_refine_maxsim(q[:3], [0, 3], pool, comp, *PARAMS[1]).shape == (1, 4)
        for bad in (np.nan, np.inf, -np.inf):  # a NaN product never compares greater: no token would be the argmax
            qb = q[:3].copy()
            qb[1, 77] = bad
            with pytest.raises(pkg.NativeError, match="finite"):
                idx.gqr_refine_maxsim(qb, [0, 3], pool, comp, *PARAMS[1])
        with pytest.raises(pkg.NativeError, match="at least one vector"):  # a query without vectors
            idx.gqr_refine_maxsim(q[:3], [0, 0, 3], np.tile(pool, (2, 1)), np.tile(comp, (2, 1)), *PARAMS[1])
        idx.remove_multivec([2])
        with pytest.raises(pkg.NativeError, match="no vectors"):  # a removed document in a pool
            idx.gqr_refine_maxsim(q[:3], [0, 3], pool, comp, *PARAMS[1])
        assert idx.gqr_refine_maxsim(q[:3], [0, 3], np.array([[0, 1, 3, -1]]), np.array([[0.5, 0.25, 0.25, 0.0]]),
                                     *PARAMS[1]).shape == (1, 4)
