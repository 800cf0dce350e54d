"""GPU: the speculative one-chunk pass behind every entry point that reaches search_block at level 0, and on
indexes that were mutated -- corpora of 65 536 rows or a few more, the smallest at which the path exists, with `spec_min_rows`
lowered to their size as in test_gpu_speculative.py.

Every case asserts bit-for-bit equality with the references the small-corpus tests of the same feature use (the oracle's
top-k, helpers.MutableOracleIndex, rows_ref / mmr_ref / groups_ref / range_ref), that the path really ran (spec_passes >= 1; the
controls one k further: spec_passes == 0 and more chunks than passes, chunk_growth = 1), and that every miss and overflow was
retried.  The counters are printed (SPEC_CALLERS ...): what a degraded sample costs is a measurement, not a contract -- whether
it retries is asserted nowhere here; exactness is."""

import groups_ref
import mmr_ref
import numpy as np
import pytest
import range_ref
import rows_ref
from helpers import MutableOracleIndex
from spec_common import PLANTED_N, PLANTED_PAIRS, arm, counters, planted_corpus, same

pytestmark = pytest.mark.gpu

N, D, NQ = 65536, 64, 48
SAMPLE = 16384


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def fresh(idx):
    """re-arm a suspended speculation (a case before may have failed more than 1 % of a block) and zero the counters"""
    idx.set_option("speculate", 1)
    idx.reset_stats()


def check(idx, label, speculates):
    st = counters(idx)
    print("SPEC_CALLERS", label, {k: v for k, v in st.items() if k != "fallback_queries"}, "suspended", idx.stat("spec_suspended"))
    assert st["retry_queries"] >= st["spec_miss_queries"] + st["spec_overflow_queries"], st
    if speculates is True:
        assert st["spec_passes"] >= 1, st
    elif speculates is False:
        assert st["spec_passes"] == 0 and st["passes"] >= 1 and st["chunks"] > st["passes"], st
    return st


def mirror(C, metric="cosine"):
    mo = MutableOracleIndex(C.shape[1], metric)
    mo.add(C)
    return mo


@pytest.fixture(scope="module")
def gauss():
    rng = np.random.default_rng(31)
    C = rng.standard_normal((N, D)).astype(np.float32)
    Q = rng.standard_normal((NQ, D)).astype(np.float32)
    C.setflags(write=False)
    Q.setflags(write=False)
    return C, Q


@pytest.fixture(scope="module")
def intact(pkg, gauss):
    """the Gaussian corpus, appended once and never mutated (MMR, groups)"""
    C, _ = gauss
    idx = pkg.Mi355Index(D)
    idx.add(C)
    arm(idx)
    yield idx
    idx.close()


# ---- by stored row -------------------------------------------------------------------------------------------------------
ROWS_REMOVED = np.array([200, 9000, 50000])


@pytest.fixture(scope="module")
def rows_case(pkg, gauss):
    C, _ = gauss
    rng = np.random.default_rng(32)
    ids = np.concatenate([rng.choice(SAMPLE, 20, replace=False), SAMPLE + rng.choice(N - SAMPLE, 22, replace=False),
                          [200, 50000], [N, N + 5, -1, 2**40]])      # in the sample, behind it, removed, outside the index
    assert len(ids) == NQ and not np.isin(ids[:42], ROWS_REMOVED).any()
    live = np.ones(N, dtype=bool)
    live[ROWS_REMOVED] = False
    idx = pkg.Mi355Index(D)
    idx.add(C)
    idx.remove_rows(ROWS_REMOVED)
    arm(idx)
    yield idx, C, ids, live
    idx.close()


@pytest.mark.parametrize("k,include_self,speculates", [(18, False, True), (19, False, False), (19, True, True), (20, True, False)])
def test_search_by_stored_row(rows_case, oracle, k, include_self, speculates):
    """self excluded, the inner pass runs at k + 1: 18 is the last k that speculates"""
    idx, C, ids, live = rows_case
    want = rows_ref.search_rows(oracle, C, ids, k, live=live, include_self=include_self)
    assert (want[1][:42, 0] >= 0).all() and (want[1][42:] == -1).all()
    fresh(idx)
    rows_ref.same(idx.search_rows(ids, k, include_self=include_self), want)
    check(idx, f"rows k={k} include_self={include_self}", speculates)


# ---- MMR -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fetch_k,speculates", [(19, True), (20, False)])
def test_mmr(intact, gauss, oracle, fetch_k, speculates):
    C, Q = gauss
    for lam in (0.0, 0.5, 1.0):
        want = mmr_ref.search_mmr(oracle, C, Q, 5, fetch_k, lam)
        fresh(intact)
        mmr_ref.same(intact.search_mmr(Q, 5, fetch_k, lam), want)
        check(intact, f"mmr fetch_k={fetch_k} lambda={lam}", speculates)


# ---- grouped search --------------------------------------------------------------------------------------------------------
def test_groups(intact, gauss, oracle):
    """groups of 1, 3 and 0 sub-queries, fetch_k = 10"""
    C, Q = gauss
    sizes = np.resize(np.array([1, 3, 0]), 36)      # 12 x (1 + 3 + 0) = 48 sub-queries
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert offs[-1] == NQ
    want = groups_ref.merge_groups(*oracle.topk_search(C, Q, 10), offs, 10)
    fresh(intact)
    groups_ref.same(intact.search_groups(Q, offs, 10, 10), want)
    check(intact, "groups fetch_k=10", True)


# ---- the range search's fallback ---------------------------------------------------------------------------------------------
def test_range_fallback(pkg, gauss, oracle):
    """a third of the queries have more rows in range than the 16 slots hold: they are searched at max_results = 10
    (an index of its own: range_slots has no way back to its default)"""
    C, Q = gauss
    slots, m = 16, 10
    ds, rs = range_ref.oracle_sorted(oracle, C, Q, depth=64)
    radius, counts = range_ref.radius_admitting(ds, rs, np.resize(np.array([7, m, slots + 9]), NQ))
    assert range_ref.covers(ds, radius) and int((counts > slots).sum()) == NQ // 3
    with pkg.Mi355Index(D) as idx:
        idx.add(C)
        arm(idx)
        idx.set_option("range_slots", slots)
        fresh(idx)
        range_ref.same(idx.search_range(Q, radius, m), range_ref.search_range(ds, rs, radius, m))
        assert idx.stat("range_fallback_queries") == NQ // 3
        check(idx, "range fallback m=10", True)


# ---- k edges, a ragged end, a row offset ---------------------------------------------------------------------------------------
def test_k_edges_on_a_ragged_corpus_with_a_row_offset(pkg, oracle):
    """n = 65 536 + 37: the one chunk ends inside a tile; ids carry 2^33; speculative exactly at k = 2 and k = 19"""
    rng = np.random.default_rng(33)
    C = rng.standard_normal((N + 37, 128)).astype(np.float32)
    Q = rng.standard_normal((NQ, 128)).astype(np.float32)
    for i in range(4):      # the best row of four queries among the 37 rows behind the last whole tile
        C[N + 9 * i] = 2.0 * Q[i]
    off = 2**33
    with pkg.Mi355Index(128) as idx:
        idx.add(C)
        idx.set_option("row_offset", off)
        arm(idx)
        for k, speculates in ((1, False), (2, True), (19, True), (20, False)):
            rd, rr = oracle.topk_search(C, Q, k)
            fresh(idx)
            got = idx.search(Q, k)
            same(got, (rd, np.where(rr >= 0, rr + off, -1)))
            check(idx, f"ragged n={N + 37} k={k}", speculates)
            assert all(got[1][i, 0] == off + N + 9 * i for i in range(4))


# ---- scattered removals and updates ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "auto"])
def test_scattered_removals_and_updates(pkg, gauss, dtype):
    """1 % of the rows removed, 1 % updated (some rescaled, one turned to zero), inside and outside the sample"""
    C, Q = gauss
    rng = np.random.default_rng(34)
    pick = rng.choice(N, 2 * 655, replace=False)
    removed, updated = pick[:655], pick[655:]
    assert (removed < SAMPLE).sum() > 100 and (updated < SAMPLE).sum() > 100
    new = rng.standard_normal((655, D)).astype(np.float32)
    new[:100] = C[updated[:100]] * np.float32(7.5)      # rescaled: the same direction
    new[100] = 0.0
    new[101] = 1.5 * Q[3]                                # a new best row
    mo = mirror(C)
    with pkg.Mi355Index(D) as idx:
        idx.set_option("screen_dtype", dtype)
        idx.add(C)
        for target in (idx, mo):
            target.remove_rows(removed)
            target.update_rows(updated, new)
        arm(idx)
        for k in (10, 19):
            fresh(idx)
            got = idx.search(Q, k)
            same(got, mo.search(Q, k))
            check(idx, f"scattered {dtype} k={k}", True)
        assert got[1][3, 0] == updated[101]
        assert not np.isin(got[1], removed).any()


# ---- the whole sample removed, then compacted --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "auto"])
def test_dead_head_then_compact(pkg, dtype):
    rng = np.random.default_rng(35)
    n = N + SAMPLE
    C = rng.standard_normal((n, D)).astype(np.float32)
    Q = rng.standard_normal((NQ, D)).astype(np.float32)
    mo = mirror(C)
    with pkg.Mi355Index(D) as idx:
        idx.set_option("screen_dtype", dtype)
        idx.add(C)
        arm(idx, N)      # (the size after the compaction below)
        for target in (idx, mo):
            target.remove_rows(np.arange(SAMPLE))
        fresh(idx)
        same(idx.search(Q, 10), mo.search(Q, 10))
        st = check(idx, f"dead head {dtype}", None)      # (overflow and retry, or no speculation: counted consistently either way)
        assert st["spec_passes"] <= 1 and st["passes"] >= 1
        if st["spec_passes"] == 0:
            assert st["retry_queries"] == 0 and st["chunks"] > st["passes"]
        suspended = idx.stat("spec_suspended")
        new_of_old = idx.compact()
        assert np.array_equal(new_of_old, mo.compact())
        assert len(idx) == N and idx.stat("spec_suspended") == 0, "compact re-arms a suspended speculation"
        idx.reset_stats()      # (NOT fresh(): the re-arming is compact's)
        same(idx.search(Q, 10), mo.search(Q, 10))
        check(idx, f"dead head {dtype}, compacted (was suspended: {suspended})", True)


# ---- ties across a removal ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lower", "upper"])
def test_ties_across_a_removal(pkg, which):
    """the planted duplicates: with the lower-row copy removed the far-end copy leads; with the upper one removed the lower alone"""
    C, Q = planted_corpus()
    lower = 100 + 37 * np.arange(PLANTED_PAIRS)
    upper = PLANTED_N - 1 - np.arange(PLANTED_PAIRS)
    gone, stays = (lower, upper) if which == "lower" else (upper, lower)
    mo = mirror(C)
    with pkg.Mi355Index(C.shape[1]) as idx:
        idx.add(C)
        arm(idx)
        for target in (idx, mo):
            target.remove_rows(gone)
        fresh(idx)
        got = idx.search(Q, 10)
        same(got, mo.search(Q, 10))
        check(idx, f"ties, {which} copies removed", True)
        assert np.array_equal(got[1][:PLANTED_PAIRS, 0], stays) and not np.isin(got[1], gone).any()


# ---- a view ------------------------------------------------------------------------------------------------------------------
def test_view_of_every_other_row(pkg, oracle):
    rng = np.random.default_rng(36)
    C = rng.standard_normal((2 * N, D)).astype(np.float32)
    Q = rng.standard_normal((NQ, D)).astype(np.float32)
    ids = np.arange(0, 2 * N, 2)

    def listed(live_ids, k):
        rd, rr = oracle.topk_search(np.ascontiguousarray(C[live_ids]), Q, k)
        return rd, np.where(rr >= 0, live_ids[np.maximum(rr, 0)], -1)

    with pkg.Mi355Index(D) as idx:
        idx.add(C)
        with idx.view(row_ids=ids) as v:
            assert len(v) == N
            arm(v)
            fresh(v)
            same(v.search(Q, 10), listed(ids, 10))
            check(v, "view of every other row", True)
        # rows of the parent's sample region removed before view(): the view's sample is of other rows, and shorter
        gone = rng.choice(2 * SAMPLE, 3000, replace=False)
        idx.remove_rows(gone)
        left = np.setdiff1d(ids, gone)
        assert 1000 < len(ids) - len(left) < 2000
        with idx.view(row_ids=ids) as v:
            assert len(v) == len(left)
            arm(v)
            fresh(v)
            same(v.search(Q, 10), listed(left, 10))
            check(v, f"view of {len(left)} rows after removals", True)


# ---- asynchronous blocks across a mutation -------------------------------------------------------------------------------------
def test_async_blocks_across_a_removal(pkg, gauss, oracle):
    """two blocks in flight, remove_rows (which drains them), a third block: each equals the corpus as it was when enqueued"""
    C, Q = gauss
    k = 10
    before = oracle.topk_search(C, Q, k)
    gone = np.unique(before[1][:, :2])      # the two best rows of every query
    mo = mirror(C)
    mo.remove_rows(gone)
    after = mo.search(Q, k)
    assert not np.array_equal(before[1], after[1])
    sel = [np.arange(0, 24), np.arange(24, 48), np.arange(12, 36)]
    with pkg.Mi355Index(D) as idx:
        idx.add(C)
        arm(idx)
        fresh(idx)
        bufs = []
        for s in sel:
            Qs = np.ascontiguousarray(Q[s])
            pq, od, orr = idx.dev_alloc(Qs.nbytes), idx.dev_alloc(len(s) * k * 8), idx.dev_alloc(len(s) * k * 8)
            idx.dev_upload(pq, Qs)
            bufs.append((pq, od, orr))
        for s, (pq, od, orr) in zip(sel[:2], bufs[:2]):
            idx.search_device_async(pq, len(s), k, od, orr)
        idx.remove_rows(gone)
        pq, od, orr = bufs[2]
        idx.search_wait(idx.search_device_async(pq, len(sel[2]), k, od, orr))
        for s, (pq, od, orr), want in zip(sel, bufs, (before, before, after)):
            gd, gr = np.empty((len(s), k)), np.empty((len(s), k), dtype=np.int64)
            idx.dev_download(od, gd)
            idx.dev_download(orr, gr)
            same((gd, gr), (want[0][s], want[1][s]))
        for b in bufs:
            for p in b:
                idx.dev_free(p)
        st = check(idx, "async across remove_rows", True)
        assert st["spec_passes"] >= 3 or idx.stat("spec_suspended") == 1
