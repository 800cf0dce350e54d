"""GPU: range search (mi355dr_search_range / Mi355Index.search_range) -- every row within a distance, counted on the device.

Every case compares ALL B x max_results distances bit for bit, all rows and all counts with tests/range_ref.py over the
oracle's all-pairs distances, on path = auto / screen / scan, screen_dtype = i8 / bf16 and both metrics.  Radii are taken from
the oracle's sorted distances, so the in-range counts are known when the case is built."""

import ctypes

import numpy as np
import pytest

import range_ref
from range_ref import same

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
INF = float("inf")
N_BASE, M = 1000, 10
SLOTS = 64           # option "range_slots" of the base cases: "more than R rows in range" fits 1000 rows
PATHS = ["auto", "screen", "scan"]
DTYPES = ["i8", "bf16"]
METRICS = ["cosine", "ip"]
SEARCH_STATS = ["passes", "chunks", "starters", "screen_launches", "fallback_queries", "retry_queries", "candidates", "rescored"]


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def configure(idx, path="auto", dtype="i8", **options):
    idx.set_option("path", path)
    idx.set_option("screen_dtype", dtype)
    for key, value in options.items():
        idx.set_option(key, value)


def base_arrays(d, seed=0):
    """1000 rows (a multiple of neither 32 nor 128) with every row class, 1030 queries with two irregular ones"""
    rng = np.random.default_rng(1000 * d + seed)
    C = rng.standard_normal((N_BASE, d)).astype(np.float32)
    C *= rng.uniform(0.5, 2.0, size=(N_BASE, 1)).astype(np.float32)
    C[5] = 0.0                                  # zero row: NaN under cosine, distance -0.0 under inner product
    C[17, 2] = np.nan                           # rows with non-finite components
    C[18, 4] = np.inf
    C[19] *= 1e20                               # huge norm: |c|^2 overflows
    C[9, 3] = 40.0 * np.abs(C[9]).max()         # one dominant component: loose under the int8 screen
    C[611, 7] = -60.0 * np.abs(C[611]).max()
    C[300] = C[301] = C[302] = C[40]            # duplicates: equal distance bits, the row decides
    Q = rng.standard_normal((1030, d)).astype(np.float32)
    Q[2] = 0.0                                  # zero query
    Q[3, 1] = np.inf                            # non-finite query
    Q[5] = C[40]                                # the duplicates are its nearest rows under cosine
    Q[7] = 1e-18 * Q[7]                         # |q|^2 below the screens' range, distances defined
    return C, Q


@pytest.fixture(scope="module")
def bases(pkg, oracle):
    """(index, C, Q, sorted all-pairs distances, their rows) per (d, metric), built once and shared read-only"""
    made = {}

    def get(d, metric):
        if (d, metric) not in made:
            C, Q = base_arrays(d)
            idx = pkg.Mi355Index(d, metric)
            idx.add(C)
            assert idx.stat("irregular_rows") >= 4 and idx.stat("loose_rows") >= idx.stat("irregular_rows") + 2
            ds, rs = range_ref.oracle_sorted(oracle, C, Q, metric)
            made[d, metric] = (idx, C, Q, ds, rs)
        return made[d, metric]

    yield get
    for idx, *_ in made.values():
        idx.close()


def wanted_counts(B, m, slots):
    """0, 1, m - 1, m, m + 1 and more than the result buffer, cycled over the queries"""
    return np.resize(np.array([m, 0, 1, m - 1, m + 1, slots + 5, 3]), B)


# ---- 1. the base shape: counts around max_results and beyond the buffer, every path, dtype, metric ------------------------------

@pytest.mark.parametrize("B", [1, 33, 130])
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", PATHS)
def test_counts_around_the_cut(bases, path, dtype, metric, d, B):
    idx, C, Q, ds, rs = bases(d, metric)
    configure(idx, path, dtype, range_slots=SLOTS, cand_cap=2048, range_chunk_rows=1 << 21)
    q0 = 8 if B == 1 else 0
    Qb, dsb, rsb = Q[q0:q0 + B], ds[q0:q0 + B], rs[q0:q0 + B]
    wants = np.array([SLOTS + 5]) if B == 1 else wanted_counts(B, M, SLOTS)
    radius, counts = range_ref.radius_admitting(dsb, rsb, wants)
    if B > 1:    # each listed count really occurs (inner product: a row with an infinite component ties at -inf for half the queries)
        assert ({0, 1, M - 1, M, M + 1} if metric == "cosine" else {M - 1, M, M + 1}) <= set(counts.tolist())
        assert (counts > SLOTS).any()
    idx.reset_stats()
    same(idx.search_range(Qb, radius, M), range_ref.search_range(dsb, rsb, radius, M))
    assert idx.stat("range_fallback_queries") == int((counts > SLOTS).sum()) > 0
    # the radius was a row's own distance bits: that row is in.  The next double below it: that row (and its ties) is out.
    below = np.nextafter(radius, -INF)
    exp = range_ref.search_range(dsb, rsb, below, M)
    moved = (counts > 0) & np.isfinite(radius)
    assert (exp[2] <= counts).all() and (exp[2][moved] < counts[moved]).all()
    same(idx.search_range(Qb, below, M), exp)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("path", PATHS)
def test_special_radii_and_a_scalar_radius(bases, path, metric):
    idx, C, Q, ds, rs = bases(100, metric)
    configure(idx, path, "i8", range_slots=4096)
    B = 33
    radius = np.resize(np.array([INF, -INF, 1e300, -1e300, 0.0, -0.0]), B)
    exp = range_ref.search_range(ds[:B], rs[:B], radius, M)
    got = idx.search_range(Q[:B], radius, M)
    same(got, exp)
    defined = (~np.isnan(ds[:B])).sum(axis=1)
    # +inf: every row with a distance; -inf: none -- but the rows AT -inf (inner product with an infinite component)
    assert np.array_equal(got[2][0::6], defined[0::6]) and np.array_equal(got[2][1::6], (ds[1:B:6] == -INF).sum(axis=1))
    assert metric == "ip" or not got[2][1::6].any()
    td, tr = idx.search(Q[:B], M)                                                      # +inf: the ordinary top-max_results
    blank = np.isnan(td[0::6])
    assert np.array_equal(got[1][0::6], np.where(blank, -1, tr[0::6]))
    assert np.array_equal(got[0][0::6][~blank].view(np.uint64), td[0::6][~blank].view(np.uint64))
    r = float(np.nanmedian(ds[:B, 20]))
    same(idx.search_range(Q[:B], r, M), range_ref.search_range(ds[:B], rs[:B], r, M))   # a scalar serves every query


# ---- 2. argument errors --------------------------------------------------------------------------------------------------------

def test_argument_errors_change_nothing(pkg, bases):
    idx, C, Q, ds, rs = bases(100, "cosine")
    configure(idx)
    before = idx.search(Q[:9], 7)
    lib, h = idx._lib, idx._h
    f32p, f64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_double, ctypes.c_int64))
    q = np.ascontiguousarray(Q[:4])
    rad = np.full(4, 0.5)
    od, orow, oc = np.empty((4, 1025)), np.empty((4, 1025), dtype=np.int64), np.empty(4, dtype=np.int64)

    def call(qa=q, B=4, ra=rad, m=5, da=od, rwa=orow, ca=oc):
        p = lambda a, t: a.ctypes.data_as(t) if a is not None else None  # noqa: E731
        return lib.mi355dr_search_range(h, p(qa, f32p), B, p(ra, f64p), m, p(da, f64p), p(rwa, i64p), p(ca, i64p))

    assert call() == 0
    stats = {key: idx.stat(key) for key in ("range_searches", "range_queries", "range_in_range")}
    assert call(ra=np.array([0.5, np.nan, 0.5, 0.5])) == E_INVALID and b"NaN" in lib.mi355dr_last_error(h)
    assert call(m=0) == E_INVALID and call(m=-3) == E_INVALID and call(B=0) == E_INVALID and call(B=-1) == E_INVALID
    assert call(m=1025) == E_UNSUPPORTED
    for null in ("qa", "ra", "da", "rwa", "ca"):
        assert call(**{null: None}) == E_INVALID
    assert call(m=1024) == 0
    with pytest.raises(ValueError):
        idx.search_range(Q[:4], np.nan, 5)
    with pytest.raises(pkg.NativeError) as e:
        idx.search_range(Q[:4], 0.5, 0)
    assert e.value.code == E_INVALID
    assert {key: idx.stat(key) for key in stats}["range_searches"] == stats["range_searches"] + 1    # (the m = 1024 call)
    after = idx.search(Q[:9], 7)
    assert np.array_equal(after[1], before[1]) and np.array_equal(after[0].view(np.uint64), before[0].view(np.uint64))


# ---- 3. ties, irregular queries ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", PATHS)
def test_duplicates_straddle_the_cut(bases, path, dtype):
    idx, C, Q, ds, rs = bases(100, "cosine")
    configure(idx, path, dtype, range_slots=4096)
    assert rs[5, :4].tolist() == [40, 300, 301, 302] and len(set(ds[5, :4].view(np.uint64).tolist())) == 1
    radius = ds[5, 0]
    d, r, c = idx.search_range(Q[5:6], radius, 2)
    assert r.tolist() == [[40, 300]] and c.tolist() == [4]              # the lower rows win, the count includes all four
    same((d, r, c), range_ref.search_range(ds[5:6], rs[5:6], radius, 2))
    same(idx.search_range(Q[5:6], radius, 3), range_ref.search_range(ds[5:6], rs[5:6], radius, 3))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", PATHS)
def test_irregular_queries(bases, path, dtype, metric):
    idx, C, Q, ds, rs = bases(100, metric)
    configure(idx, path, dtype, range_slots=4096)
    sel = [2, 3, 7, 0]                                                   # zero, non-finite, tiny norm, an ordinary one
    radius = np.array([INF, INF, 0.0, 0.0])
    if metric == "cosine":
        radius[2:] = 0.97
    exp = range_ref.search_range(ds[sel], rs[sel], radius, M)
    same(idx.search_range(Q[sel], radius, M), exp)
    if metric == "cosine":
        assert exp[2][:2].tolist() == [0, 0] and exp[2][2] > 0           # no distance is defined for the first two
    for one in range(3):                                                 # ... and alone in a block
        same(idx.search_range(Q[sel[one]], radius[one], M), range_ref.search_range(ds[sel[one]][None], rs[sel[one]][None], radius[one], M))


# ---- 4. removed, updated and compacted rows -----------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
def test_removed_updated_compacted(pkg, oracle, metric):
    d, B = 100, 40
    C, Q = base_arrays(d, seed=1)
    Q = Q[:B]
    rng = np.random.default_rng(8)
    near = range_ref.oracle_sorted(oracle, C, Q, metric)[1]
    removed = np.unique(np.concatenate([near[:10, 0], near[10:20, 2], rng.choice(N_BASE, 60, replace=False), [5, 9]]))
    updated = np.setdiff1d(rng.choice(N_BASE, 50, replace=False), removed)
    new_rows = rng.standard_normal((len(updated), d)).astype(np.float32)
    new_rows[0] = Q[11]                                                  # an updated row becomes a query's nearest
    C2 = C.copy()
    C2[updated] = new_rows
    live = np.ones(N_BASE, dtype=bool)
    live[removed] = False
    ds, rs = range_ref.oracle_sorted(oracle, C2, Q, metric)
    radius, counts = range_ref.radius_admitting(ds, rs, wanted_counts(B, M, SLOTS), live)
    assert (counts > SLOTS).any() and (counts == M + 1).any()
    exp = range_ref.search_range(ds, rs, radius, M, live)
    keep = np.flatnonzero(live)
    dsc, rsc = range_ref.oracle_sorted(oracle, C2[keep], Q, metric)
    exp_c = range_ref.search_range(dsc, rsc, radius, M)
    assert np.array_equal(exp_c[2], exp[2]) and np.array_equal(np.where(exp_c[1] >= 0, keep[np.maximum(exp_c[1], 0)], -1), exp[1])
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(C)
        idx.remove_rows(removed)
        idx.update_rows(updated, new_rows)
        for path in PATHS:
            for dtype in DTYPES:
                configure(idx, path, dtype, range_slots=SLOTS)
                same(idx.search_range(Q, radius, M), exp)
        idx.compact()
        for path in PATHS:
            configure(idx, path, "i8", range_slots=SLOTS)
            same(idx.search_range(Q, radius, M), exp_c)


# ---- 5. kernel reach: several chunks, a ragged last chunk, every screen kernel -----------------------------------------------

N_REACH, D_REACH, DEPTH = 20_000, 128, 400
_REACH = {}


def reach_case(oracle):
    if not _REACH:
        rng = np.random.default_rng(20)
        C = rng.standard_normal((N_REACH, D_REACH)).astype(np.float32)
        C[4100] = 0.0
        C[8200, 3] = 50.0 * np.abs(C[8200]).max()
        C[19_990, 9] = np.nan
        Q = rng.standard_normal((1024, D_REACH)).astype(np.float32)
        Q[100] = 0.0
        ds, rs = range_ref.oracle_sorted(oracle, C, Q, depth=DEPTH)
        radius, counts = range_ref.radius_admitting(ds, rs, np.resize(np.array([10, 0, 1, 100, 150, 11, 37]), 1024))
        assert range_ref.covers(ds, radius)
        exp = range_ref.search_range(ds, rs, radius, M)
        for a in (*exp, radius):
            a.setflags(write=False)
        _REACH.update(C=C, Q=Q, radius=radius, exp=exp)
    return _REACH["C"], _REACH["Q"], _REACH["radius"], _REACH["exp"]


@pytest.fixture(scope="module")
def reach(pkg, oracle):
    C, Q, radius, exp = reach_case(oracle)
    with pkg.Mi355Index(D_REACH) as idx:
        idx.add(C)
        yield idx, Q, radius, exp


REACH_SETS = {                                    # the option sets of tests/test_gpu_screen_hits.py
    "rq-130": (130, "i8", dict(small_chunk_rows=0, screen_rq=1)),
    "rq-1024": (1024, "i8", dict(small_chunk_rows=0, screen_rq=1)),
    "256c-i8-130": (130, "i8", dict(small_chunk_rows=0, screen_rq=0)),
    "256c-bf16-1024": (1024, "bf16", dict(small_chunk_rows=0)),
    "stream-40": (40, "i8", dict(screen_stream=1)),
    "stream-bf16-64": (64, "bf16", dict(screen_stream=1)),
    "tile-130": (130, "i8", dict(small_chunk_rows=16384, screen_stream=0)),
    "tile-bf16-40": (40, "bf16", dict(small_chunk_rows=16384, screen_stream=0)),
}


@pytest.mark.parametrize("case", list(REACH_SETS))
def test_every_screen_kernel_over_chunks(reach, case):
    idx, Q, radius, exp = reach
    B, dtype, options = REACH_SETS[case]
    configure(idx, "screen", dtype, range_slots=4096, cand_cap=2048, screen_rq=1, screen_stream=1, small_chunk_rows=16384)
    configure(idx, "screen", dtype, range_chunk_rows=4096, **options)       # 4 whole chunks and a ragged fifth
    idx.reset_stats()
    got = idx.search_range(Q[:B], radius[:B], M)
    same(got, tuple(a[:B] for a in exp))
    assert idx.stat("range_candidates") >= idx.stat("range_rescored") >= int(exp[2][:B].sum()) - 1
    assert idx.stat("range_fallback_queries") == 0
    assert (idx.stat("screen_rq_launches") > 0) == case.startswith("rq")
    idx.set_option("range_chunk_rows", 1 << 21)                             # the default: one launch over all rows
    again = idx.search_range(Q[:B], radius[:B], M)
    same(again, got)


def test_exact_path_over_chunks(reach):
    idx, Q, radius, exp = reach
    for scan_dma in (1, 0):
        configure(idx, "scan", "i8", range_chunk_rows=4096, range_slots=4096, scan_dma=scan_dma)
        same(idx.search_range(Q[:70], radius[:70], M), tuple(a[:70] for a in exp))
    idx.set_option("scan_dma", 1)


# ---- 6. candidate-list overflow on the screen path ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_screen_overflow_is_redone_exactly(pkg, oracle, dtype):
    """2048 near-copies of one direction, lists of 16 slots, a radius that admits a quarter of the rows: every chunk overflows
    every list, and every (query, chunk) pair is served by the exact range scan in list-sized pieces"""
    rng = np.random.default_rng(31)
    d, n_dense, B = 128, 2048, 40
    axis = rng.standard_normal(d).astype(np.float32)
    C = (axis[None, :] + 0.05 * rng.standard_normal((n_dense + 256, d))).astype(np.float32)
    C[n_dense:] = rng.standard_normal((256, d)).astype(np.float32)
    Q = (axis[None, :] + 0.05 * rng.standard_normal((B, d))).astype(np.float32)
    ds, rs = range_ref.oracle_sorted(oracle, C, Q)
    radius, counts = range_ref.radius_admitting(ds, rs, len(C) // 4)
    assert (counts == len(C) // 4).all()
    exp = range_ref.search_range(ds, rs, radius, 100)
    with pkg.Mi355Index(d) as idx:
        idx.add(C)
        configure(idx, "screen", dtype, cand_cap=16, range_chunk_rows=1024)
        same(idx.search_range(Q, radius, 100), exp)
        assert idx.stat("range_redo_chunks") >= B and idx.stat("range_fallback_queries") == 0
        idx.reset_stats()
        idx.set_option("range_slots", 128)                # ... and with the buffer below the count: the counts alone stand
        same(idx.search_range(Q, radius, 100), exp)
        assert idx.stat("range_fallback_queries") == B and idx.stat("range_redo_chunks") > 0
        rd, rr = oracle.topk_search(C, Q[:5], 10)         # the index still searches
        got = idx.search(Q[:5], 10)
        assert np.array_equal(got[1], rr) and np.array_equal(got[0], rd)


# ---- 7. internal blocks, state hygiene, views, offsets, the device form, stats --------------------------------------------------

@pytest.mark.parametrize("path", ["auto", "scan"])
def test_internal_blocks(bases, path):
    idx, C, Q, ds, rs = bases(100, "cosine")
    configure(idx, path, "i8", range_slots=SLOTS)
    radius, counts = range_ref.radius_admitting(ds, rs, wanted_counts(1030, M, SLOTS))
    same(idx.search_range(Q, radius, M), range_ref.search_range(ds, rs, radius, M))


@pytest.mark.parametrize("path", PATHS)
def test_a_search_is_the_same_before_and_after(bases, path):
    idx, C, Q, ds, rs = bases(768, "cosine")
    configure(idx, path, "i8", range_slots=SLOTS)
    B = 130
    radius, _ = range_ref.radius_admitting(ds[:B], rs[:B], wanted_counts(B, M, SLOTS))
    before = [idx.search(Q[:B], k) for k in (10, 100)]
    exp = range_ref.search_range(ds[:B], rs[:B], radius, M)
    same(idx.search_range(Q[:B], radius, M), exp)
    for (bd, br), k in zip(before, (10, 100)):
        ad, ar = idx.search(Q[:B], k)
        assert np.array_equal(ar, br) and np.array_equal(ad.view(np.uint64), bd.view(np.uint64))
    # a range call issued while an asynchronous block is in flight completes that block first, correctly
    k = 10
    Qa = np.ascontiguousarray(Q[200:330])
    pq, od, orr = idx.dev_alloc(Qa.nbytes), idx.dev_alloc(len(Qa) * k * 8), idx.dev_alloc(len(Qa) * k * 8)
    try:
        idx.dev_upload(pq, Qa)
        ticket = idx.search_device_async(pq, len(Qa), k, od, orr)
        same(idx.search_range(Q[:B], radius, M), exp)
        idx.search_wait(ticket)
        gd, gr = np.empty((len(Qa), k)), np.empty((len(Qa), k), dtype=np.int64)
        idx.dev_download(od, gd)
        idx.dev_download(orr, gr)
    finally:
        for p in (pq, od, orr):
            idx.dev_free(p)
    assert np.array_equal(gr, rs[200:330, :k]) and np.array_equal(gd.view(np.uint64), ds[200:330, :k].view(np.uint64))


@pytest.mark.parametrize("metric", METRICS)
def test_views_and_row_offset(pkg, oracle, bases, metric):
    idx, C, Q, ds, rs = bases(100, metric)
    rng = np.random.default_rng(77)
    ids = np.sort(rng.choice(N_BASE, size=333, replace=False))
    ids = np.union1d(ids, [5, 9, 17, 40, 300, 302])
    B = 33
    dv, rv = range_ref.oracle_sorted(oracle, C[ids], Q[:B], metric)
    radius, counts = range_ref.radius_admitting(dv, rv, wanted_counts(B, M, SLOTS))
    ed, er, ec = range_ref.search_range(dv, rv, radius, M)
    er = np.where(er >= 0, ids[np.maximum(er, 0)], -1)                      # under the parent's ids
    with idx.view(row_ids=ids) as v:
        for path in PATHS:
            configure(v, path, "i8", range_slots=SLOTS)
            same(v.search_range(Q[:B], radius, M), (ed, er, ec))
    configure(idx, "auto", "i8", range_slots=SLOTS, row_offset=5_000_000_000)
    try:
        radius, _ = range_ref.radius_admitting(ds[:B], rs[:B], wanted_counts(B, M, SLOTS))
        ed, er, ec = range_ref.search_range(ds[:B], rs[:B], radius, M)
        same(idx.search_range(Q[:B], radius, M), (ed, np.where(er >= 0, er + 5_000_000_000, -1), ec))
    finally:
        idx.set_option("row_offset", 0)


@pytest.mark.parametrize("path", ["auto", "scan"])
def test_device_form(bases, path):
    idx, C, Q, ds, rs = bases(768, "ip")
    configure(idx, path, "i8", range_slots=SLOTS)
    B = 130
    Qb = np.ascontiguousarray(Q[:B])
    radius, _ = range_ref.radius_admitting(ds[:B], rs[:B], wanted_counts(B, M, SLOTS))
    pq, od, orr, oc = idx.dev_alloc(Qb.nbytes), idx.dev_alloc(B * M * 8), idx.dev_alloc(B * M * 8), idx.dev_alloc(B * 8)
    try:
        idx.dev_upload(pq, Qb)
        idx.search_range_device(pq, B, radius, M, od, orr, oc)                # stream = NULL: the index's own
        gd, gr, gc = np.empty((B, M)), np.empty((B, M), dtype=np.int64), np.empty(B, dtype=np.int64)
        idx.dev_download(od, gd)
        idx.dev_download(orr, gr)
        idx.dev_download(oc, gc)
    finally:
        for p in (pq, od, orr, oc):
            idx.dev_free(p)
    same((gd, gr, gc), range_ref.search_range(ds[:B], rs[:B], radius, M))


def test_stats(bases):
    idx, C, Q, ds, rs = bases(100, "cosine")
    configure(idx, "auto", "i8", range_slots=4096)
    B = 130
    radius, counts = range_ref.radius_admitting(ds[:B], rs[:B], wanted_counts(B, M, SLOTS))
    idx.search(Q[:B], M)
    idx.reset_stats()
    got = idx.search_range(Q[:B], radius, M)
    assert idx.stat("range_searches") == 1 and idx.stat("range_queries") == B
    assert idx.stat("range_in_range") == int(got[2].sum()) == int(counts.sum())
    assert idx.stat("range_candidates") >= idx.stat("range_rescored") > 0 and idx.stat("range_fallback_queries") == 0
    assert idx.stat("range_redo_chunks") >= 2      # the two irregular queries of the block took the exact path
    assert not any(idx.stat(key) for key in SEARCH_STATS)                   # nothing of the ordinary search moved
    idx.search_range(Q[:7], radius[:7], 3)
    assert idx.stat("range_searches") == 2 and idx.stat("range_queries") == B + 7
    idx.set_option("path", "scan")
    idx.reset_stats()
    idx.search_range(Q[:B], radius, M)
    assert idx.stat("range_candidates") == idx.stat("range_rescored") == 0 and idx.stat("range_in_range") == int(counts.sum())
    assert not any(idx.stat(key) for key in SEARCH_STATS)
    for key, bad in (("range_chunk_rows", 255), ("range_slots", 15), ("range_slots", 4097)):
        with pytest.raises(Exception, match=key):
            idx.set_option(key, bad)
    idx.reset_stats()
    assert idx.stat("range_searches") == 0 and idx.stat("range_in_range") == 0
