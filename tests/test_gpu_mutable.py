"""GPU: the mutable single-vector index -- update_rows / remove_rows in place.

Every expectation comes from the CPU oracle alone: `oracle.topk_search` over the compacted matrix of the LIVE rows in
their current values, its row numbers mapped back through the list of live ids (compaction keeps the ids ascending, so
the oracle's tie-break by row is the index's tie-break by id).  Ids and float8 distance bits must match (NaN positions,
not NaN payloads).  The order (distance asc, NaN last, row asc) is total, so the answer at (B, k) is the corner
[:B, :k] of the answer at (300, 300): the oracle runs once per matrix version and metric (`Expect`)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = [10, 100, 300]
BS = [1, 64, 300]            # streaming, tile and register-query screens
METRICS = ["cosine", "ip"]
DTYPES = ["auto", "bf16", "i8"]
PATHS = ["screen", "scan"]
SIZES = [(200_000, 768), (50_000, 100)]   # (100: a dim that is not a multiple of 32)
QMAX, KMAX = 300, 300


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def gauss(seed, n, d):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


class Expect:
    """The oracle's answer over the live rows of C for up to QMAX queries and k <= kmax, computed once."""

    def __init__(self, oracle, C, live_ids, Q, metric, kmax=KMAX):
        live_ids = np.asarray(live_ids, dtype=np.int64)
        assert np.all(np.diff(live_ids) > 0)
        full = live_ids.shape[0] == C.shape[0]
        d, r = oracle.topk_search(C if full else C[live_ids], Q, kmax, metric=metric)
        self.dist, self.rows = d, np.where(r >= 0, live_ids[np.maximum(r, 0)], -1)

    def at(self, B, k):
        return self.dist[:B, :k], self.rows[:B, :k]


def same(got, exp, what=""):
    (dg, rg), (de, re_) = got, exp
    assert np.array_equal(rg, re_), f"ids differ {what}"
    assert np.array_equal(np.isnan(dg), np.isnan(de)), f"NaN positions differ {what}"
    ok = ~np.isnan(dg)
    assert np.array_equal(dg[ok].view(np.uint64), de[ok].view(np.uint64)), f"distance bits differ {what}"


def check_grid(idx, exp, Q, ks=KS, bs=BS, dtypes=DTYPES, paths=PATHS, dead=None, what=""):
    for path in paths:
        idx.set_option("path", path)
        for dt in dtypes:
            idx.set_option("screen_dtype", dt)
            for B in bs:
                for k in ks:
                    got = idx.search(Q[:B], k)
                    same(got, exp.at(B, k), f"({what} path={path} screen_dtype={dt} B={B} k={k})")
                    if dead is not None:
                        assert not np.isin(got[1], dead).any(), f"a removed id came back ({what} {path} {dt} B={B} k={k})"
    idx.set_option("path", "auto")
    idx.set_option("screen_dtype", "auto")


def rogue(rows, seed):
    """one outlier component per row: peak * sqrt(d) far above 6 (outside the int8 residual limit)"""
    rng = np.random.default_rng(seed)
    out = rows.copy()
    out[np.arange(out.shape[0]), rng.integers(0, out.shape[1], size=out.shape[0])] += 40.0
    return out


def class_counts(oracle, C, live):
    """(irregular, loose) live rows as the library defines them (dev_common.h): irregular = |c|^2 (the fp32 chain) outside
    [1e-30, 1e30]; loose = irregular or a component with |c_k| / |c| > 6 / sqrt(d).  The inputs keep clear of the limit."""
    n2 = oracle.row_nrm2(C).astype(np.float64)
    with np.errstate(invalid="ignore"):
        regular = (n2 >= 1e-30) & (n2 <= 1e30)
    peak = np.zeros(C.shape[0])
    peak[regular] = np.abs(C[regular].astype(np.float64)).max(axis=1) / np.sqrt(n2[regular])
    lim = 6.0 / np.sqrt(C.shape[1])
    assert not (np.abs(peak[regular] / lim - 1.0) < 0.02).any(), "test input too close to the loose-row limit"
    live_mask = np.zeros(C.shape[0], bool)
    live_mask[live] = True
    irregular = ~regular & live_mask
    loose = (irregular | (regular & (peak > lim))) & live_mask
    return int(irregular.sum()), int(loose.sum())


# ---- 1. update parity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,d", SIZES)
def test_update_parity(pkg, oracle, n, d, metric):
    rng = np.random.default_rng([1, n, d])
    C = gauss([10, n, d], n, d)
    Q = gauss([11, n, d], QMAX, d)
    ids = rng.choice(n, size=n // 20, replace=False)
    new = gauss([12, n, d], ids.shape[0], d)
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(C)
        for part in np.array_split(np.arange(ids.shape[0]), 3):   # three calls
            idx.update_rows(ids[part], new[part])
        C[ids] = new
        assert len(idx) == n and idx.live_rows == n and idx.stat("dead_rows") == 0
        check_grid(idx, Expect(oracle, C, np.arange(n), Q, metric), Q, what=f"update n={n} d={d} {metric}")


# ---- 2. update equals add -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,d", [(40_013, 768), (20_000, 100)])
def test_update_equals_add(pkg, oracle, n, d, metric):
    rng = np.random.default_rng([2, n, d])
    old = gauss([20, n, d], n, d)
    Q = gauss([21, n, d], QMAX, d)
    ids = rng.choice(n, size=n // 20, replace=False)
    new = gauss([22, n, d], ids.shape[0], d)
    new[:8] = rogue(new[:8], 23)          # some rows change class on the way
    new[8:12] = 0.0
    final = old.copy()
    final[ids] = new
    n_groups = (n + 31) // 32
    with pkg.Mi355Index(d, metric) as a, pkg.Mi355Index(d, metric) as b:
        a.add(final)
        b.add(old)
        half = ids.shape[0] // 2
        b.update_rows(ids[:half], new[:half])
        dev = b.dev_alloc(new[half:].nbytes)           # the second half through the device entry point
        b.dev_upload(dev, new[half:])
        b.update_rows_device(ids[half:], dev)
        b.dev_free(dev)
        assert np.array_equal(a.get_rows(0, n).view(np.uint32), b.get_rows(0, n).view(np.uint32))
        for key in ("irregular_rows", "loose_rows", "dead_rows"):
            assert a.stat(key) == b.stat(key), key
        assert (a.stat("irregular_rows"), a.stat("loose_rows")) == class_counts(oracle, final, np.arange(n))
        assert a.stat("irregular_rows") == 4 and a.stat("loose_rows") >= 12
        for ix in (a, b):
            ix.set_option("screen_dtype", "i8")
        sa, sb = a.debug_i8_state(Q[:4], 0, n_groups), b.debug_i8_state(Q[:4], 0, n_groups)
        for x, y, name in zip(sa, sb, ("S_q", "kq", "S_g", "e_g")):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
        touched = np.unique(ids // 32)
        assert (sa[2][touched] > 0).all()
        for path in PATHS:
            for dt in DTYPES:
                for B, k in ((1, 10), (64, 100), (300, 10), (300, 300)):
                    for ix in (a, b):
                        ix.set_option("path", path)
                        ix.set_option("screen_dtype", dt)
                    same(b.search(Q[:B], k), a.search(Q[:B], k), f"(update vs add {path} {dt} B={B} k={k})")


# ---- 3. class changes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,d,ks", [(20_000, 128, [10, 100]), (700, 64, [10, 710])])
def test_class_changes(pkg, oracle, n, d, ks, metric):
    rng = np.random.default_rng([3, n, d])
    C = gauss([30, n, d], n, d)
    Q = gauss([31, n, d], 200, d)
    pick = rng.choice(n, size=90, replace=False)
    to_zero, to_nan, to_rogue = pick[:20], pick[20:40], pick[40:70]
    live = np.arange(n)
    base = class_counts(oracle, C, live)[1]   # (Gaussian rows that happen to be loose: a 6-sigma component, usually none)
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(C)

        def step(ids, rows, what):
            idx.update_rows(ids, rows)
            C[ids] = rows
            irr, loose = class_counts(oracle, C, live)
            assert (idx.stat("irregular_rows"), idx.stat("loose_rows")) == (irr, loose), what
            # (the oracle puts NaN distances last, by row: irregular rows come back last with NaN where k reaches them)
            check_grid(idx, Expect(oracle, C, live, Q, metric, kmax=max(ks)), Q, ks=ks, bs=[5, 200], what=f"{what} n={n} {metric}")
            return irr, loose - base

        assert step(to_zero, np.zeros((20, d), np.float32), "regular -> zero") == (20, 20)
        bad = gauss(32, 20, d)
        bad[np.arange(20), rng.integers(0, d, size=20)] = np.nan
        assert step(to_nan, bad, "regular -> NaN component") == (40, 40)
        assert step(np.concatenate([to_zero, to_nan]), gauss(33, 40, d), "irregular -> regular") == (0, 0)
        assert step(to_rogue, rogue(gauss(34, 30, d), 35), "tight -> rogue") == (0, 30)
        assert step(to_rogue, gauss(36, 30, d), "rogue -> tight") == (0, 0)


# ---- 4. remove parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,d", [(200_013, 768), (50_009, 100)])   # (a partly filled last group of 32)
def test_remove_parity(pkg, oracle, n, d, metric):
    rng = np.random.default_rng([4, n, d])
    C = gauss([40, n, d], n, d)
    Q = gauss([41, n, d], QMAX, d)
    _, top = oracle.topk_search(C, Q, 10, metric=metric)       # the answer BEFORE the removal
    g = int(rng.integers(1, n // 32 - 1))
    dead = np.unique(np.concatenate([
        rng.choice(n, size=n // 10, replace=False),            # a random 10 %
        np.arange(32 * g, 32 * g + 32),                        # one whole aligned group
        np.arange(n // 32 * 32, n),                            # every row of the last, partly filled group
        top[::7, :3].ravel(), top[5, :],                       # rows in the top-10 of some query
    ]))
    live = np.setdiff1d(np.arange(n), dead)
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(C)
        for part in np.array_split(rng.permutation(dead), 2):
            idx.remove_rows(part)
        assert len(idx) == n
        assert idx.live_rows == live.shape[0] and idx.stat("dead_rows") == dead.shape[0]
        check_grid(idx, Expect(oracle, C, live, Q, metric), Q, dead=dead, what=f"remove n={n} d={d} {metric}")
        dot, dist = idx.debug_rescore(Q[:2], [0, 1], [int(dead[0]), int(dead[-1])])
        assert np.isnan(dot).all() and np.isnan(dist).all()


# ---- 5. removal is not irregularity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_removed_rows_are_not_irregular_rows(pkg, oracle, metric):
    n, d, B, k = 100_000, 128, 64, 10
    C = gauss(50, n, d)
    C[[5, 77]] = 0.0                       # two irregular rows and three loose ones that stay
    C[[9, 1000, 4242]] = rogue(C[[9, 1000, 4242]], 51)
    Q = gauss(52, B, d)
    dead = np.random.default_rng(53).choice(np.arange(100, n), size=5000, replace=False)   # well above kIrrCap = 1024
    live = np.setdiff1d(np.arange(n), dead)
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(C)
        idx.search(Q, k)
        before = {key: idx.stat(key) for key in ("irregular_rows", "loose_rows", "screen_dtype_active")}
        assert (before["irregular_rows"], before["loose_rows"]) == class_counts(oracle, C, np.arange(n))
        assert before["irregular_rows"] == 2 and before["loose_rows"] >= 5
        idx.remove_rows(dead)
        exp = Expect(oracle, C, live, Q, metric, kmax=k)
        for path in ("auto", "screen"):
            idx.set_option("path", path)
            idx.reset_stats()
            same(idx.search(Q, k), exp.at(B, k), f"({path})")
            assert idx.stat("screen_launches") > 0 and idx.stat("fallback_queries") == 0, path
            assert {key: idx.stat(key) for key in before} == before, path
        assert idx.stat("dead_rows") == 5000


# ---- 6. few live rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_few_live_rows(pkg, oracle, metric):
    n, d, k = 6_000, 64, 10
    C = gauss(60, n, d)
    Q = gauss(61, 70, d)
    live = np.sort(np.random.default_rng(62).choice(n, size=7, replace=False))
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(C)
        idx.remove_rows(np.setdiff1d(np.arange(n), live))
        assert idx.live_rows == 7
        exp = Expect(oracle, C, live, Q, metric, kmax=k)
        assert (exp.rows[:, :7] >= 0).all() and (exp.rows[:, 7:] == -1).all() and np.isnan(exp.dist[:, 7:]).all()
        check_grid(idx, exp, Q, ks=[k], bs=[1, 70], what=f"7 live rows {metric}")
        idx.remove_rows(live)
        assert idx.live_rows == 0 and len(idx) == n
        for path in PATHS:
            for dt in DTYPES:
                idx.set_option("path", path)
                idx.set_option("screen_dtype", dt)
                dist, rows = idx.search(Q, k)       # (rc OK: a failure raises)
                assert (rows == -1).all() and np.isnan(dist).all(), (path, dt)


# ---- 7. revive, no-op, errors -------------------------------------------------------------------------------------------------------
def test_revive_noop_and_errors(pkg, oracle):
    n, d, B, k = 10_000, 128, 40, 10
    C = gauss(70, n, d)
    Q = gauss(71, B, d)
    _, top = oracle.topk_search(C, Q, k)
    victim = int(top[0, 0])
    others = np.unique(np.array([3, 64, int(top[1, 0])], dtype=np.int64))
    others = others[others != victim]
    with pkg.Mi355Index(d, "cosine") as idx:
        idx.add(C)
        idx.remove_rows(np.concatenate([[victim], others]))
        live = np.setdiff1d(np.arange(n), np.concatenate([[victim], others]))
        exp_removed = Expect(oracle, C, live, Q, "cosine", kmax=k)
        same(idx.search(Q, k), exp_removed.at(B, k), "(removed)")
        idx.remove_rows([victim])                      # a second remove of a dead row changes nothing
        assert idx.live_rows == n - 1 - others.shape[0]
        same(idx.search(Q, k), exp_removed.at(B, k), "(removed twice)")
        new = gauss(72, 1, d)
        idx.update_rows([victim], new)                 # revive by update
        C[victim] = new[0]
        live = np.setdiff1d(np.arange(n), others)
        exp = Expect(oracle, C, live, Q, "cosine", kmax=k)
        assert idx.live_rows == live.shape[0]
        check_grid(idx, exp, Q, ks=[k], bs=[B], what="revived")
        idx.update_rows([victim], C[victim:victim + 1] * 0 + Q[0])    # ... and it can win again
        C[victim] = Q[0]
        got = idx.search(Q, k)
        assert got[1][0, 0] == victim
        same(got, Expect(oracle, C, live, Q, "cosine", kmax=k).at(B, k), "(revived, best)")
        before = idx.search(Q, k)
        for bad in ([n], [-1], [5, 9, 5]):
            with pytest.raises(pkg.NativeError) as e:
                idx.remove_rows(bad)
            assert e.value.code == -1
            with pytest.raises(pkg.NativeError) as e:
                idx.update_rows(bad, gauss(73, len(bad), d))
            assert e.value.code == -1
            assert idx.live_rows == live.shape[0]
            same(idx.search(Q, k), before, f"(after rejected ids {bad})")


# ---- 8. append after mutate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_append_after_mutate(pkg, oracle, metric):
    n, d, extra = 20_013, 128, 10_000          # 20 013 = 625 groups + 13 rows: the append lands in a partly filled group
    rng = np.random.default_rng(80)
    C = gauss(81, n, d)
    Q = gauss(82, 200, d)
    dead = np.unique(np.concatenate([rng.choice(n, size=900, replace=False), [n - 1, n - 5, n - 13]]))
    upd = np.setdiff1d(rng.choice(n, size=700, replace=False), dead[::2])   # (some updates revive dead rows)
    new = gauss(83, upd.shape[0], d)
    more = gauss(84, extra, d)
    more[:3] = rogue(more[:3], 85)
    more[3] = 0.0
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(C)
        idx.remove_rows(dead)
        idx.update_rows(upd, new)
        idx.add(more)
        C[upd] = new
        C = np.concatenate([C, more])
        gone = np.setdiff1d(dead, upd)
        live = np.setdiff1d(np.arange(n + extra), gone)
        assert len(idx) == n + extra and idx.live_rows == live.shape[0] and idx.stat("dead_rows") == gone.shape[0]
        assert (idx.stat("irregular_rows"), idx.stat("loose_rows")) == class_counts(oracle, C, live)
        assert idx.stat("irregular_rows") == 1 and idx.stat("loose_rows") >= 4
        check_grid(idx, Expect(oracle, C, live, Q, metric, kmax=100), Q, ks=[10, 100], bs=[1, 200], dead=gone,
                   what=f"append after mutate {metric}")


# ---- 9. async ordering ------------------------------------------------------------------------------------------------------------------
def test_async_search_then_update(pkg, oracle):
    n, d, B, k = 60_000, 128, 300, 10
    C = gauss(90, n, d)
    Q = gauss(91, B, d)
    exp_before = Expect(oracle, C, np.arange(n), Q, "cosine", kmax=k)
    ids = np.unique(exp_before.rows[:, 0])                     # every query's best row is replaced ...
    new = -C[ids]                                              # ... by its opposite
    with pkg.Mi355Index(d, "cosine") as idx:
        idx.add(C)
        q_dev, od, orow = idx.dev_alloc(Q.nbytes), idx.dev_alloc(B * k * 8), idx.dev_alloc(B * k * 8)
        idx.dev_upload(q_dev, Q)
        ticket = idx.search_device_async(q_dev, B, k, od, orow)
        idx.update_rows(ids, new)                              # no wait in between
        idx.search_wait(ticket)
        dist, rows = np.empty((B, k), np.float64), np.empty((B, k), np.int64)
        idx.dev_download(od, dist)
        idx.dev_download(orow, rows)
        same((dist, rows), exp_before.at(B, k), "(the ticket: the matrix before the update)")
        C[ids] = new
        exp_after = Expect(oracle, C, np.arange(n), Q, "cosine", kmax=k)
        assert not np.array_equal(exp_after.rows[:, 0], exp_before.rows[:, 0])
        same(idx.search(Q, k), exp_after.at(B, k), "(a search after the update)")
        for p in (q_dev, od, orow):
            idx.dev_free(p)


# ---- 10. row shards: removed rows never come back through the merge ---------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_removed_rows_stay_out_of_a_sharded_merge(pkg, oracle, metric):
    """Two row shards with global ids (`row_offset`), searched on device and merged by the shard-merge kernel as a
    row-sharded search does.  The second shard keeps 4 live rows: its lists end in a NaN / -1 tail the merge must skip."""
    n, d, B, k, cut = 30_000, 128, 50, 10, 18_000
    C = gauss(100, n, d)
    Q = gauss(101, B, d)
    _, top = oracle.topk_search(C, Q, k, metric=metric)
    keep2 = cut + np.sort(np.random.default_rng(102).choice(n - cut, size=4, replace=False))
    dead = np.unique(np.concatenate([np.setdiff1d(np.arange(cut, n), keep2), top[top < cut][::3],
                                     np.random.default_rng(103).choice(cut, size=2000, replace=False)]))
    live = np.setdiff1d(np.arange(n), dead)
    with pkg.Mi355Index(d, metric) as s0, pkg.Mi355Index(d, metric) as s1:
        s0.add(C[:cut])
        s1.add(C[cut:])
        s1.set_option("row_offset", cut)
        s0.remove_rows(dead[dead < cut])
        s1.remove_rows(dead[dead >= cut] - cut)
        assert s0.live_rows + s1.live_rows == live.shape[0] and s1.live_rows == 4
        dist_all, rows_all = np.empty((2, B, k), np.float64), np.empty((2, B, k), np.int64)
        for w, s in enumerate((s0, s1)):
            q_dev, od, orow = s.dev_alloc(Q.nbytes), s.dev_alloc(B * k * 8), s.dev_alloc(B * k * 8)
            s.dev_upload(q_dev, Q)
            s.search_device(q_dev, B, k, od, orow)
            s.dev_download(od, dist_all[w])
            s.dev_download(orow, rows_all[w])
            for p in (q_dev, od, orow):
                s.dev_free(p)
        assert (rows_all[1][:, 4:] == -1).all() and (rows_all[1][:, :4] >= cut).all()
        pd, pr = s0.dev_alloc(dist_all.nbytes), s0.dev_alloc(rows_all.nbytes)
        od, orow = s0.dev_alloc(B * k * 8), s0.dev_alloc(B * k * 8)
        s0.dev_upload(pd, dist_all)
        s0.dev_upload(pr, rows_all)
        s0.merge_topk_device(pd, pr, 2, B, k, od, orow)
        s0.synchronize()
        got = np.empty((B, k), np.float64), np.empty((B, k), np.int64)
        s0.dev_download(od, got[0])
        s0.dev_download(orow, got[1])
        for p in (pd, pr, od, orow):
            s0.dev_free(p)
        same(got, Expect(oracle, C, live, Q, metric, kmax=k).at(B, k), f"(sharded merge {metric})")
        assert not np.isin(got[1], dead).any()
