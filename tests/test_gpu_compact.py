"""GPU: compaction of the single-vector index -- `Mi355Index.compact()` drops the removed rows in place.

The yardstick is always a FRESH `Mi355Index` built by one `add` of the live rows in their order, plus the CPU oracle over
those rows: the compacted index must return the same ids and the same float8 distance bits (NaN positions, not payloads) on
every path and screen dtype, and must show the same rows, classes, int8 group records and dense screen values."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1000
KS = [1, 10, 100]
BS = [1, 64, 128, 200]       # k_screen_stream, k_screen and the large-block screens all read the rebuilt tail
SLICES = [32, 96, None]      # compact_slice_rows (None: the default)
PATHS = ["auto", "screen", "scan"]
DTYPES = ["auto", "i8", "bf16"]
METRICS = ["cosine", "ip"]
PATTERNS = ["none", "row0", "last", "group1", "last700", "every2nd", "random10", "all"]


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def gauss(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def removed_of(pattern, n):
    return {"none": np.zeros(0, np.int64), "row0": np.array([0]), "last": np.array([n - 1]), "group1": np.arange(32, 64),
            "last700": np.arange(n - 700, n), "every2nd": np.arange(0, n, 2),
            "random10": np.sort(np.random.default_rng(3).choice(n, n // 10, replace=False)), "all": np.arange(n)}[pattern]


def expected_map(n, removed):
    live = np.ones(n, bool)
    live[removed] = False
    return np.where(live, np.cumsum(live) - 1, -1).astype(np.int64), np.nonzero(live)[0]


def same(got, exp, what=""):
    (dg, rg), (de, re_) = got, exp
    assert np.array_equal(rg, re_), f"ids differ {what}"
    assert np.array_equal(np.isnan(dg), np.isnan(de)), f"NaN positions differ {what}"
    ok = ~np.isnan(dg)
    assert np.array_equal(dg[ok].view(np.uint64), de[ok].view(np.uint64)), f"distance bits differ {what}"


def answers(pkg, idx, Q, ks=KS, bs=BS, paths=PATHS, dtypes=DTYPES):
    """every search of the grid, options back at auto afterwards.  No shape of this file may be refused: every index here has
    at most 1 024 rows outside either shadow when it is searched, so both screens serve, and a NativeError fails the test."""
    out = {}
    for path in paths:
        idx.set_option("path", path)
        for dt in dtypes:
            idx.set_option("screen_dtype", dt)
            for B in bs:
                for k in ks:
                    out[path, dt, B, k] = idx.search(Q[:B], k)
    idx.set_option("path", "auto")
    idx.set_option("screen_dtype", "auto")
    return out


def state(pkg, idx, Q):
    """what the readers other than the searches show"""
    n = len(idx)
    s = {"len": n, "live": idx.live_rows}
    for key in ("dead_rows", "irregular_rows", "loose_rows", "screen_dtype_active"):
        s[key] = idx.stat(key)
    if n:
        s["rows"] = idx.get_rows(0, n).view(np.uint32)
        idx.set_option("screen_dtype", "i8")     # (the group records are shown while the int8 screen is the active one)
        s["i8_state"] = np.concatenate([a.view(np.uint32) for a in idx.debug_i8_state(Q[:4], 0, (n + 31) // 32)])
        idx.set_option("screen_dtype", "auto")
        s["dense"] = idx.debug_screen_dense(Q[:8], 0, min(n, 2048))
    return s


def same_state(got, exp, what=""):
    assert got.keys() == exp.keys(), what
    for key in exp:
        assert np.array_equal(got[key], exp[key], equal_nan=key == "dense"), f"{key} differs {what}"


class Fresh:
    """a fresh index over C (one add), its answers and state, and the oracle's word on the auto path"""

    def __init__(self, pkg, oracle, C, Q, metric, **grid):
        self.idx = pkg.Mi355Index(C.shape[1], metric)
        if C.shape[0]:
            self.idx.add(C)
        self.answers = answers(pkg, self.idx, Q, **grid)
        self.state = state(pkg, self.idx, Q)
        ks, bs = grid.get("ks", KS), grid.get("bs", BS)
        if C.shape[0] == 0:
            return
        d, r = oracle.topk_search(C, Q[:max(bs)], max(ks), metric=metric)
        for B in bs:
            for k in ks:
                same(self.answers["auto", "auto", B, k], (d[:B, :k], r[:B, :k]), f"(fresh index vs oracle B={B} k={k})")

    def close(self):
        self.idx.close()


def check_equal(pkg, idx, fresh, Q, what, **grid):
    got = answers(pkg, idx, Q, **grid)
    for key, exp in fresh.answers.items():
        same(got[key], exp, f"({what} path={key[0]} screen_dtype={key[1]} B={key[2]} k={key[3]})")
    same_state(state(pkg, idx, Q), fresh.state, what)


# ---- 1. removal patterns ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [5, 30, 64, 768])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_removal_patterns(pkg, oracle, pattern, d, metric):
    C = gauss([1, d], N, d)
    Q = gauss([2, d], max(BS), d)
    removed = removed_of(pattern, N)
    exp_map, live = expected_map(N, removed)
    fresh = Fresh(pkg, oracle, C[live], Q, metric)
    try:
        for sl in SLICES:
            what = f"{pattern} d={d} {metric} slice={sl}"
            with pkg.Mi355Index(d, metric) as idx:
                idx.add(C)
                if removed.size:
                    idx.remove_rows(removed)
                if sl is not None:
                    idx.set_option("compact_slice_rows", sl)
                idx.reset_stats()
                got_map = idx.compact()
                assert got_map.dtype == np.int64 and np.array_equal(got_map, exp_map), what
                assert len(idx) == idx.live_rows == live.size and idx.stat("dead_rows") == 0, what
                first_dead = int(removed.min()) if removed.size else N
                moved = int((live > first_dead).sum())
                assert idx.stat("compact_moved_rows") == moved and idx.stat("compactions") == (1 if moved else 0), what
                check_equal(pkg, idx, fresh, Q, what)
                if pattern == "all":       # size 0: nothing to return; then an add, and the index is a fresh one again
                    dist, rows = idx.search(Q[:3], 5)
                    assert np.isnan(dist).all() and (rows == -1).all()
                    idx.add(C[:300])
                    again = Fresh(pkg, oracle, C[:300], Q, metric)
                    try:
                        check_equal(pkg, idx, again, Q, what + " + add")
                    finally:
                        again.close()
    finally:
        fresh.close()


# ---- 2. special rows ------------------------------------------------------------------------------------------------------------
def rogue(rows, seed):
    """one outlier component per row: far outside the int8 residual limit (a loose row)"""
    rng = np.random.default_rng(seed)
    out = rows.copy()
    out[np.arange(out.shape[0]), rng.integers(0, out.shape[1], size=out.shape[0])] += 40.0
    return out


@pytest.mark.parametrize("metric", METRICS)
def test_zero_rows_back_under_the_cap(pkg, oracle, metric):
    """1 100 zero rows are more than the screens tolerate (1 024); 200 of them are removed: the compacted index lists 900 under
    their new ids and screens again, exactly like the fresh index"""
    n, d = 5000, 64
    rng = np.random.default_rng(21)
    C = gauss(20, n, d)
    zeros = np.sort(rng.choice(n, 1100, replace=False))
    C[zeros] = 0.0
    removed = np.sort(np.concatenate([rng.choice(zeros, 200, replace=False),
                                      rng.choice(np.setdiff1d(np.arange(n), zeros), 300, replace=False)]))
    exp_map, live = expected_map(n, removed)
    Q = gauss(22, 200, d)
    grid = dict(ks=[10, 1000], bs=[1, 64, 200])
    fresh = Fresh(pkg, oracle, C[live], Q, metric, **grid)
    try:
        with pkg.Mi355Index(d, metric) as idx:
            idx.add(C)
            idx.remove_rows(removed)
            idx.set_option("compact_slice_rows", 96)
            assert np.array_equal(idx.compact(), exp_map)
            assert idx.stat("irregular_rows") == 900 == fresh.idx.stat("irregular_rows")
            check_equal(pkg, idx, fresh, Q, f"zero rows {metric}", **grid)
            # (the active dtype follows the k of the last search: compared behind the same searches on both indexes)
            assert idx.stat("screen_dtype_active") == fresh.idx.stat("screen_dtype_active")
            for ix in (idx, fresh.idx):
                ix.reset_stats()
                ix.search(Q[:64], 10)
            assert idx.stat("fallback_queries") == fresh.idx.stat("fallback_queries")
    finally:
        fresh.close()


@pytest.mark.parametrize("metric", METRICS)
def test_special_rows_between_removed_ones(pkg, oracle, metric):
    """live zero / NaN / Inf rows and loose rows (an outlier component) between removed rows"""
    n, d = N, 64
    C = gauss(30, n, d)
    C[10:40:3] = 0.0
    C[41, 3] = np.nan
    C[500, 0] = np.inf
    C[501] = -np.inf
    C[33:36] = rogue(C[33:36], 31)
    C[600:640:2] = rogue(C[600:640:2], 32)
    C[990:] = 0.0
    removed = np.unique(np.concatenate([np.arange(11, 40, 3), np.arange(36, 41), np.arange(490, 500), np.arange(601, 640, 2),
                                        [502, 995]]))
    irregular = np.setdiff1d(np.concatenate([np.setdiff1d(np.arange(10, 40, 3), [34]), [41, 500, 501], np.arange(990, n)]), removed)
    exp_map, live = expected_map(n, removed)
    Q = gauss(33, 200, d)
    grid = dict(ks=[10, 1000], bs=[1, 64, 200])       # (k = 1000 is above the live count: the special rows come back, last)
    fresh = Fresh(pkg, oracle, C[live], Q, metric, **grid)
    try:
        for sl in (32, None):
            with pkg.Mi355Index(d, metric) as idx:
                idx.add(C)
                idx.remove_rows(removed)
                if sl is not None:
                    idx.set_option("compact_slice_rows", sl)
                assert np.array_equal(idx.compact(), exp_map)
                assert idx.stat("irregular_rows") > 0 and idx.stat("loose_rows") > idx.stat("irregular_rows")
                assert idx.stat("irregular_rows") == irregular.size
                check_equal(pkg, idx, fresh, Q, f"special rows {metric} slice={sl}", **grid)
                if metric == "cosine":                          # last, with NaN, under their NEW ids
                    dist, rows = idx.search(Q[:1], 1000)
                    assert rows[0][np.isnan(dist[0]) & (rows[0] >= 0)].tolist() == exp_map[irregular].tolist()
    finally:
        fresh.close()


# ---- 3. ties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_ties_break_by_new_id(pkg, oracle, metric):
    n, d = N, 30
    C = gauss(40, n, d)
    C[[5, 70, 300, 301, 650, 999]] = C[2]         # duplicates on both sides of the removed rows
    C[[64, 400, 800]] = C[63]
    removed = np.array([3, 4, 69, 299, 302, 649, 700, 998])
    exp_map, live = expected_map(n, removed)
    Q = gauss(41, 64, d)
    Q[0], Q[1] = C[2], C[63]
    grid = dict(ks=[10, 100], bs=[1, 64])
    fresh = Fresh(pkg, oracle, C[live], Q, metric, **grid)
    try:
        with pkg.Mi355Index(d, metric) as idx:
            idx.add(C)
            idx.remove_rows(removed)
            idx.set_option("compact_slice_rows", 32)
            assert np.array_equal(idx.compact(), exp_map)
            check_equal(pkg, idx, fresh, Q, f"ties {metric}", **grid)
            if metric == "cosine":
                assert idx.search(Q[:1], 7)[1][0].tolist() == exp_map[[2, 5, 70, 300, 301, 650, 999]].tolist()
    finally:
        fresh.close()


# ---- 4. dead head -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slice_rows", [None, 4096])
def test_dead_head(pkg, oracle, slice_rows):
    """the oldest 70 000 of 100 000 rows removed: after compact() the passes run like a fresh index's (default slice: one
    slice; 4 096: eight slices, the last one partial)"""
    n, d, dead = 100_000, 64, 70_000
    C = gauss(50, n, d)
    Q = gauss(51, 256, d)
    grid = dict(ks=[10, 100], bs=[64, 256], paths=["auto"], dtypes=["auto"])
    fresh = Fresh(pkg, oracle, C[dead:], Q, "cosine", **grid)
    try:
        with pkg.Mi355Index(d) as idx:
            idx.add(C)
            idx.remove_rows(np.arange(dead))
            if slice_rows is not None:
                idx.set_option("compact_slice_rows", slice_rows)
            exp_map = np.concatenate([np.full(dead, -1), np.arange(n - dead)])
            assert np.array_equal(idx.compact(), exp_map)
            assert idx.stat("compact_moved_rows") == n - dead
            got = answers(pkg, idx, Q, **grid)
            for key, exp in fresh.answers.items():
                same(got[key], exp, f"(dead head {key})")
            for B in (64, 256):
                for k in (10, 100):
                    for ix in (idx, fresh.idx):
                        ix.reset_stats()
                        ix.search(Q[:B], k)
                    for key in ("retry_queries", "fallback_queries"):
                        assert idx.stat(key) == fresh.idx.stat(key), (key, B, k)
    finally:
        fresh.close()


# ---- 5. life goes on ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_life_goes_on(pkg, oracle, metric):
    n, d = N, 64
    C = gauss(60, n, d)
    Q = gauss(61, 200, d)
    grid = dict(ks=[10, 100], bs=[1, 64, 200], paths=["auto", "scan"])

    def equal_fresh(idx, M, what):
        fresh = Fresh(pkg, oracle, M, Q, metric, **grid)
        try:
            check_equal(pkg, idx, fresh, Q, what, **grid)
        finally:
            fresh.close()

    with pkg.Mi355Index(d, metric) as idx:
        idx.add(C)
        removed = removed_of("random10", n)
        idx.remove_rows(removed)
        idx.set_option("compact_slice_rows", 96)
        idx.compact()
        M = C[expected_map(n, removed)[1]]                      # 900 rows: the last group holds 4
        more = gauss(62, 77, d)
        idx.add(more)                                           # into the partly filled last group
        M = np.concatenate([M, more])
        equal_fresh(idx, M, f"add after compact {metric}")
        ids = np.array([0, 31, 450, 899, 900, 976])
        M[ids] = gauss(63, ids.size, d)
        idx.update_rows(ids, M[ids])
        equal_fresh(idx, M, f"update after compact {metric}")
        gone = np.array([1, 2, 3, 500, 975])
        idx.remove_rows(gone)
        assert len(idx) == 977 and idx.live_rows == 972
        exp_map, live = expected_map(977, gone)
        assert np.array_equal(idx.compact(), exp_map)           # the second compaction
        M = M[live]
        equal_fresh(idx, M, f"second compact {metric}")
        idx.remove_rows(np.arange(10, 972))
        assert np.array_equal(idx.compact(), expected_map(972, np.arange(10, 972))[0])
        dist, rows = idx.search(Q[:5], 30)                      # k above the live count: NaN / -1 tail
        rd, rr = oracle.topk_search(M[:10], Q[:5], 30, metric=metric)
        same((dist, rows), (rd, rr), "(k above the live count)")
        assert (rows[:, 10:] == -1).all() and np.isnan(dist[:, 10:]).all()


# ---- 6. a search in flight ------------------------------------------------------------------------------------------------------------
def test_search_in_flight_completes_under_old_ids(pkg, oracle):
    n, d, B, k = 20_000, 64, 64, 10
    C = gauss(70, n, d)
    Q = gauss(71, B, d)
    removed = np.arange(0, n, 3)
    exp_map, live = expected_map(n, removed)
    with pkg.Mi355Index(d) as idx:
        idx.add(C)
        idx.remove_rows(removed)
        pq, od, orr = idx.dev_alloc(Q.nbytes), idx.dev_alloc(B * k * 8), idx.dev_alloc(B * k * 8)
        idx.dev_upload(pq, Q)
        ticket = idx.search_device_async(pq, B, k, od, orr)
        got_map = idx.compact()                                 # (not waited for: the call completes the block first)
        idx.search_wait(ticket)
        gd, gr = np.empty((B, k)), np.empty((B, k), dtype=np.int64)
        idx.dev_download(od, gd)
        idx.dev_download(orr, gr)
        rd, rr = oracle.topk_search(C[live], Q, k)
        same((gd, gr), (rd, live[rr]), "(in flight: old ids)")
        assert np.array_equal(got_map, exp_map)
        same(idx.search(Q, k), (rd, rr), "(after the compaction: new ids)")
        for p in (pq, od, orr):
            idx.dev_free(p)


# ---- 7. arguments ---------------------------------------------------------------------------------------------------------------------
def test_arguments(pkg):
    from autorag_research_amd import _native

    lib = _native.load()
    C = gauss(80, 100, 8)
    idx = pkg.Mi355Index(8)
    idx.add(C)
    idx.remove_rows([5, 50])
    assert lib.mi355dr_compact(idx._h, None) == 0               # a NULL map is accepted
    assert len(idx) == idx.live_rows == 98
    assert np.array_equal(idx.get_rows(0, 98), np.delete(C, [5, 50], axis=0))
    assert lib.mi355dr_compact(None, None) != 0                 # a NULL handle is refused
    for bad in (31, 0, -1, (1 << 22) + 1):
        with pytest.raises(pkg.NativeError):
            idx.set_option("compact_slice_rows", bad)
    idx.set_option("compact_slice_rows", 32)
    idx.set_option("compact_slice_rows", 1 << 22)
    idx.close()
    with pytest.raises(ValueError):
        idx.compact()                                           # a closed handle is refused


# ---- the service over the real library ----------------------------------------------------------------------------------------------
def test_service_unit_compacts_and_answers_like_a_fresh_service(pkg):
    from autorag_research_amd.service import Mi355RetrievalService
    from autorag_research_amd.store import ChunkTable, InMemoryStore

    n, d = 600, 32
    emb = gauss(90, n, d)
    ids = [f"pk{i:04d}" for i in range(n)]
    Q = gauss(91, 5, d)

    def service(e, keys):
        store = InMemoryStore()
        store.chunks = ChunkTable(ids=list(keys), contents=[f"text {pk}" for pk in keys], embedding=e.copy())
        return Mi355RetrievalService(lambda: store)

    def ask(s):
        return [s.vector_search_by_embedding(q.tolist(), top_k=20) for q in Q]

    s = service(emb, ids)
    ask(s)                                                      # builds the unit
    emb1 = emb.copy()
    emb1[np.arange(0, n, 4)] = np.nan
    emb1[7] = Q[0]
    more = gauss(92, 9, d)
    t1 = ChunkTable(ids=ids + [f"new{i}" for i in range(9)], contents=[""] * (n + 9), embedding=np.concatenate([emb1, more]))
    t1.contents = [f"text {pk}" for pk in t1.ids]
    assert s.refresh_unit("chunk", t1) == "incremental"
    unit = s._units["chunk"]
    handle = unit.single
    assert s.compact_unit("chunk") and unit.single is handle
    assert len(handle) == handle.live_rows == n + 9 - 150 and handle.stat("compactions") == 1
    f = service(t1.embedding, t1.ids)
    try:
        assert ask(s) == ask(f)
        emb2 = t1.embedding.copy()                              # ... and the compacted unit keeps following in place
        emb2[[1, 2]] = np.nan
        emb2[9] = Q[1]
        t2 = ChunkTable(ids=list(t1.ids), contents=list(t1.contents), embedding=emb2)
        assert s.refresh_unit("chunk", t2) == "incremental" and unit.single is handle
        f2 = service(emb2, t1.ids)
        try:
            assert ask(s) == ask(f2)
        finally:
            f2.close()
    finally:
        f.close()
        s.close()
