"""GPU: the speculative one-chunk pass -- one screen launch over all rows at a threshold the starter's sample
predicts, verified against the pass's own k-th best.  Whatever the model gets right or wrong, every block equals the CPU
oracle: ids and the bits of the float64 distances.  Corpora are the smallest the path exists at (the starter needs 4 samples of
16 384 rows), with `spec_min_rows` lowered to their size."""

import numpy as np
import pytest
from spec_common import index as _index
from spec_common import planted_corpus
from spec_common import same as _same

pytestmark = pytest.mark.gpu

N, K = 65536, 10


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


# ---- Gaussian rows: the model holds ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauss(oracle):
    """(C, Q, oracle answer) per (d, metric), computed once"""
    out = {}
    for d, metric, seed in ((128, "cosine", 11), (128, "ip", 12), (64, "cosine", 13)):
        rng = np.random.default_rng(seed)
        C = rng.standard_normal((N, d)).astype(np.float32)
        Q = rng.standard_normal((600, d)).astype(np.float32)
        out[d, metric] = (C, Q, oracle.topk_search(C, Q, K, metric=metric))
    return out


@pytest.mark.parametrize("d,metric", [(128, "cosine"), (128, "ip"), (64, "cosine")])
def test_engagement_and_parity(pkg, gauss, d, metric):
    C, Q, (rd, rr) = gauss[d, metric]
    with _index(pkg, C, metric) as idx:
        for B in (600, 40):  # (the large-block screens; the small-block one)
            for dtype in ("auto", "bf16"):
                idx.set_option("screen_dtype", dtype)
                idx.set_option("speculate", 1)
                idx.reset_stats()
                got = idx.search(Q[:B], K)
                st = {s: idx.stat(s) for s in ("spec_passes", "passes", "chunks", "spec_miss_queries", "spec_overflow_queries",
                                               "retry_queries", "fallback_queries")}
                print(d, metric, B, dtype, st, "candidates", idx.stat("candidates"))
                _same(got, (rd[:B], rr[:B]))
                assert st["passes"] == 1 and st["spec_passes"] == st["passes"] and st["chunks"] == st["passes"], st
                assert st["spec_miss_queries"] == st["spec_overflow_queries"] == st["retry_queries"] == 0, st
                idx.set_option("speculate", 0)
                idx.reset_stats()
                ladder = idx.search(Q[:B], K)
                assert np.array_equal(ladder[1], got[1]) and np.array_equal(ladder[0].view(np.uint64), got[0].view(np.uint64))
                assert idx.stat("spec_passes") == 0 and idx.stat("chunks") > idx.stat("passes")


@pytest.fixture(scope="module")
def wide(oracle):
    """A corpus of 64 samples, for the model that is too LOW: the published threshold is max(rigorous, model), so what a low model
    leaves is the sample's rigorous threshold, and that admits about k * (n / sample) * inflation candidates -- 400 at four
    samples, which every list holds.  Lists overflow only where that product passes their size: 2^20 rows give ~700 candidates
    per query (spread ~30 %: the k-th best of a sample is a tenth order statistic) against the 784 slots the test leaves them --
    the fewest with which k = 10 may speculate at all (10 m <= 0.75 (slots - k)).  d = 128, not less: the model's Gaussian
    quantile is derived at d = 768, and at this n the lighter tails of d <= 64 leave it under 3 standard deviations of margin
    (tools/spec_model.py margin())."""
    rng = np.random.default_rng(14)
    C = rng.standard_normal((1 << 20, 128), dtype=np.float32)
    Q = rng.standard_normal((64, 128)).astype(np.float32)
    return C, Q, oracle.topk_search(C, Q, K)


@pytest.mark.parametrize("shift,counter", [(1500, "spec_miss_queries"), (-3000, "spec_overflow_queries")])
def test_wrong_model_is_caught_and_suspends_speculation(pkg, gauss, wide, shift, counter):
    """the threshold 1.5 standard deviations too high: the k-th best does not justify it; 3 too low: the lists overflow"""
    C, Q, (rd, rr) = gauss[128, "cosine"] if shift > 0 else wide
    with _index(pkg, C) as idx:
        if shift < 0:  # the fewest slots with which k = 10 may speculate, from the compiled-in m(10): 784 at m = 58
            from autorag_research_amd import _native

            idx.set_option("cand_cap", -(-40 * _native.load().mi355dr_debug_spec_m(K) // 3) + K)
        idx.reset_stats()
        _same(idx.search(Q[:40], K), (rd[:40], rr[:40]))
        assert idx.stat("spec_passes") == 1 and idx.stat("retry_queries") == 0  # (the model as it is holds on this corpus)
        dtype_before = idx.stat("screen_dtype_active")
        idx.set_option("spec_shift_milli", shift)
        idx.reset_stats()
        _same(idx.search(Q, K), (rd, rr))
        print(shift, {s: idx.stat(s) for s in ("spec_miss_queries", "spec_overflow_queries", "retry_queries", "fallback_queries")})
        assert idx.stat("spec_passes") == 1 and idx.stat(counter) > 0
        assert idx.stat("retry_queries") >= idx.stat("spec_miss_queries") + idx.stat("spec_overflow_queries")  # (they are retried)
        assert idx.stat("i8_demoted") == 0 and idx.stat("screen_dtype_active") == dtype_before
        assert idx.stat("spec_suspended") == 1
        # suspended: the next 16 first attempts take the ladder, then the index speculates again
        for i in range(16):
            idx.reset_stats()
            _same(idx.search(Q[:40], K), (rd[:40], rr[:40]))
            assert idx.stat("spec_passes") == 0 and idx.stat("chunks") > idx.stat("passes"), i
        assert idx.stat("spec_suspended") == 0
        idx.set_option("spec_shift_milli", 0)
        idx.reset_stats()
        _same(idx.search(Q[:40], K), (rd[:40], rr[:40]))
        assert idx.stat("spec_passes") == 1 and idx.stat("retry_queries") == 0
        # a block that fails again suspends again; setting the option ends it
        idx.set_option("spec_shift_milli", shift)
        _same(idx.search(Q[:40], K), (rd[:40], rr[:40]))
        assert idx.stat("spec_suspended") == 1
        idx.set_option("speculate", 1)
        assert idx.stat("spec_suspended") == 0


def test_a_k_without_an_admissible_m_keeps_the_ladder(pkg, gauss, oracle):
    C, Q, _ = gauss[64, "cosine"]
    with _index(pkg, C) as idx:
        idx.reset_stats()
        _same(idx.search(Q[:40], 24), oracle.topk_search(C, Q[:40], 24))
        assert idx.stat("spec_passes") == 0 and idx.stat("starters") == 1 and idx.stat("chunks") > 1


# ---- data the model is wrong about, no shift ------------------------------------------------------------------------------
D2 = 64


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


@pytest.fixture(scope="module")
def hard(oracle):
    """three corpora with their queries and oracle answers"""
    out = {}
    # (a) the best rows of some queries inside the sample, each with an exact duplicate at the far end (tie: lower row first);
    # zero rows; a row the int8 shadow cannot hold; a zero query and a NaN query
    C, Q = planted_corpus()
    out["planted"] = (C, Q)
    # (b) a dense cluster of 3000 rows around 8 queries, behind the sample
    rng = np.random.default_rng(22)
    C = rng.standard_normal((N, D2)).astype(np.float32)
    centre = _unit(rng.standard_normal(D2))
    C[40000:43000] = (centre + 0.03 * rng.standard_normal((3000, D2))).astype(np.float32)
    Q = rng.standard_normal((48, D2)).astype(np.float32)
    Q[8:16] = (centre + 0.03 * rng.standard_normal((8, D2))).astype(np.float32)
    out["cluster"] = (C, Q)
    # (c) a corpus sorted by similarity to query 0, best first: the sample is the head of the distribution
    rng = np.random.default_rng(23)
    C = rng.standard_normal((N, D2)).astype(np.float32)
    Q = rng.standard_normal((48, D2)).astype(np.float32)
    C = np.ascontiguousarray(C[np.argsort(-(_unit(C) @ _unit(Q[0])), kind="stable")])
    out["sorted"] = (C, Q)
    return {name: (C, Q, oracle.topk_search(C, Q, K)) for name, (C, Q) in out.items()}


@pytest.mark.parametrize("name", ["planted", "cluster", "sorted"])
@pytest.mark.parametrize("dtype", ["auto", "bf16"])
def test_data_the_model_is_wrong_about(pkg, hard, name, dtype):
    C, Q, want = hard[name]
    with _index(pkg, C) as idx:
        idx.set_option("screen_dtype", dtype)
        idx.reset_stats()
        got = idx.search(Q, K)
        print(name, dtype, {s: idx.stat(s) for s in ("spec_passes", "spec_miss_queries", "spec_overflow_queries", "retry_queries",
                                                     "fallback_queries", "loose_rows", "irregular_rows")})
        _same(got, want)
        assert idx.stat("spec_passes") == 1
        if name == "planted":  # the duplicates tie: the lower row leads
            assert all(got[1][i, 0] == 100 + 37 * i and got[1][i, 1] == N - 1 - i for i in range(8))


def test_four_asynchronous_blocks_in_flight(pkg, hard):
    """the second block holds the cluster queries: its fix-ups run at the wait, behind the blocks enqueued after it"""
    C, Q, (rd, rr) = hard["cluster"]
    with _index(pkg, C) as idx:
        idx.reset_stats()
        sel = [np.r_[0:8, 16:32], np.r_[8:16, 32:40], np.r_[24:48], np.r_[0:8, 40:48]]
        bufs, tickets = [], []
        for s in sel:
            Qs = np.ascontiguousarray(Q[s])
            pq, od, orr = idx.dev_alloc(Qs.nbytes), idx.dev_alloc(len(s) * K * 8), idx.dev_alloc(len(s) * K * 8)
            idx.dev_upload(pq, Qs)
            bufs.append((pq, od, orr))
            tickets.append(idx.search_device_async(pq, len(s), K, od, orr))
        idx.search_wait(tickets[-1])
        for s, (pq, od, orr) in zip(sel, bufs):
            gd, gr = np.empty((len(s), K)), np.empty((len(s), K), dtype=np.int64)
            idx.dev_download(od, gd)
            idx.dev_download(orr, gr)
            _same((gd, gr), (rd[s], rr[s]))
            for p in (pq, od, orr):
                idx.dev_free(p)
        # every block was enqueued before the first wait, so all four speculated; the cluster queries of the second one fail
        # (3000 rows above any threshold the sample predicts) and suspend what comes later -- once, not once per block
        assert idx.stat("spec_passes") == 4
        assert idx.stat("spec_overflow_queries") + idx.stat("spec_miss_queries") >= 8 and idx.stat("spec_suspended") == 1
        for i in range(16):
            idx.search(Q[:8], K)
        assert idx.stat("spec_suspended") == 0
