"""GPU: search by stored row (mi355dr_search_rows / mi355dr_search_range_rows and their Python wrappers) -- the neighbours of
stored rows, the row itself left out, the query vectors read on the device.

Every case compares ALL B x k distances bit for bit, all rows and all counts with tests/rows_ref.py over the oracle's
distances."""

import ctypes

import numpy as np
import pytest

import range_ref
import rows_ref
from rows_ref import same

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
INF = float("inf")
N_BASE, M = 1000, 10
SLOTS = 64           # option "range_slots" of the range cases: "more than R rows in range" fits 1000 rows
PATHS = ["auto", "screen", "scan"]
DTYPES = ["i8", "bf16"]
METRICS = ["cosine", "ip"]
ALWAYS = [5, 17, 18, 19, 9, 40, 300, 302]   # zero row, NaN / inf / 1e20 rows, a loose row, three of the four duplicates
DUPS = [40, 300, 301, 302]


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def configure(idx, path="auto", dtype="i8", **options):
    idx.set_option("path", path)
    idx.set_option("screen_dtype", dtype)
    for key, value in options.items():
        idx.set_option(key, value)


def base_rows(d, seed=0):
    """the 1000-row corpus of the range tests (a multiple of neither 32 nor 128) with every row class"""
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
    C.setflags(write=False)
    return C


def draw_ids(B, seed=0):
    """B ids with repeats; from 8 slots up always the special rows"""
    if B == 1:
        return np.array([302], dtype=np.int64)
    rng = np.random.default_rng(B + seed)
    ids = np.concatenate([ALWAYS, rng.integers(0, N_BASE, size=B - len(ALWAYS))]).astype(np.int64)
    ids[-1] = ids[-2]                            # at least one id twice
    return ids


@pytest.fixture(scope="module")
def bases(pkg):
    """(index, C) per (d, metric), built once and shared; every test sets the options it depends on"""
    made = {}

    def get(d, metric):
        if (d, metric) not in made:
            C = base_rows(d)
            idx = pkg.Mi355Index(d, metric)
            idx.add(C)
            assert idx.stat("irregular_rows") >= 4 and idx.stat("loose_rows") >= idx.stat("irregular_rows") + 2
            made[d, metric] = (idx, C)
        return made[d, metric]

    yield get
    for idx, _ in made.values():
        idx.close()


@pytest.fixture(scope="module")
def ref(oracle):
    """the reference's answers, computed once per case and shared read-only among the paths and screen types"""
    made = {}

    def get(kind, C, key, *args, **kw):
        if (kind, key) not in made:
            out = getattr(rows_ref, kind)(oracle, C, *args, **kw)
            for a in out:
                a.setflags(write=False)
            made[kind, key] = out
        return made[kind, key]

    return get


def wanted_counts(B, m, slots):
    """0, 1, m - 1, m, m + 1 and more than the result buffer, cycled over the slots"""
    return np.resize(np.array([m, 0, 1, m - 1, m + 1, slots + 5, 3]), B)


# ---- 1. the base shape ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 33, 130])
@pytest.mark.parametrize("d", [100, 768])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", PATHS)
def test_base_shape(bases, ref, path, dtype, metric, d, B):
    idx, C = bases(d, metric)
    configure(idx, path, dtype, cand_cap=2048)
    ids = draw_ids(B)
    for k in (1, 10):
        for include_self in (False, True):
            exp = ref("search_rows", C, (d, metric, B, k, include_self), ids, k, metric, None, include_self)
            got = idx.search_rows(ids, k, include_self=include_self)
            same(got, exp)
            if include_self:     # exactly the ordinary search of the stored vectors
                sd, sr = idx.search(np.ascontiguousarray(C[ids]), k)
                assert np.array_equal(got[1], sr) and np.array_equal(got[0].view(np.uint64), sd.view(np.uint64))
            else:
                assert not (got[1] == ids[:, None]).any()


# ---- 2. the duplicate corner: the smallest shape at which the drop can go wrong ---------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", PATHS)
def test_duplicate_corner(bases, oracle, path, dtype, metric):
    idx, C = bases(100, metric)
    configure(idx, path, dtype, range_slots=SLOTS)
    cosine = metric == "cosine"
    if cosine:   # the premise: the four copies are each other's nearest rows, the lowest ids first
        assert oracle.topk_search(C, C[302:303], 4, metric=metric)[1][0].tolist() == DUPS
    for row, k in ((302, 2), (302, 3), (40, 1), (301, 2), (300, 1)):
        got = idx.search_rows([row], k)
        same(got, rows_ref.search_rows(oracle, C, [row], k, metric))
        if cosine:
            assert got[1][0].tolist() == [r for r in DUPS if r != row][:k]
    # the range form: the radius is the duplicates' own distance bits, then the next double below it
    dup = oracle.topk_search(np.ascontiguousarray(C[40:41]), C[302:303], 1, metric=metric)[0][0, 0]
    ids = np.array([302, 40, 301], dtype=np.int64)
    for m in (1, 2, 3):
        for include_self in (False, True):
            got = idx.search_range_rows(ids, dup, m, include_self=include_self)
            same(got, rows_ref.search_range_rows(oracle, C, ids, dup, m, metric, None, include_self))
            if cosine:
                assert got[2].tolist() == [4 if include_self else 3] * 3
            below = np.nextafter(dup, -INF)
            got = idx.search_range_rows(ids, below, m, include_self=include_self)
            same(got, rows_ref.search_range_rows(oracle, C, ids, below, m, metric, None, include_self))
            if cosine:
                assert got[2].tolist() == [0, 0, 0]


# ---- 3. class boundaries of the inner pass -------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [31, 32, 127, 128, 1023])
@pytest.mark.parametrize("path", ["auto", "scan"])
def test_class_boundaries(bases, ref, path, k):
    idx, C = bases(100, "cosine")
    configure(idx, path, "i8", cand_cap=2048)
    ids = draw_ids(33)
    got = idx.search_rows(ids, k)
    same(got, ref("search_rows", C, ("bound", k), ids, k, "cosine"))
    if k == 1023:    # more than the live rows: the NaN / -1 tail
        assert (got[1][:, N_BASE - 1:] == -1).all() and np.isnan(got[0][:, N_BASE - 1:]).all() and (got[1][:, 0] >= 0).all()


def test_k_1024_needs_include_self(pkg, bases, ref):
    idx, C = bases(100, "cosine")
    configure(idx, "auto", "i8", cand_cap=2048)
    ids = draw_ids(33)
    before = idx.search_rows(ids, 7)
    stats = {key: idx.stat(key) for key in ("rows_searches", "rows_queries", "rows_skipped", "passes")}
    with pytest.raises(pkg.NativeError) as e:
        idx.search_rows(ids, 1024)
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(pkg.NativeError) as e:
        idx.search_range_rows(ids, 0.5, 1024)
    assert e.value.code == E_UNSUPPORTED
    assert {key: idx.stat(key) for key in stats} == stats
    same(idx.search_rows(ids, 7), before)
    same(idx.search_rows(ids, 1024, include_self=True), ref("search_rows", C, ("k1024",), ids, 1024, "cosine", None, True))
    with pytest.raises(pkg.NativeError) as e:
        idx.search_rows(ids, 1025, include_self=True)
    assert e.value.code == E_UNSUPPORTED


# ---- 4. hygiene: ids outside the index, row_offset, refusals ---------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
def test_ids_outside_the_index(bases, oracle, metric):
    idx, C = bases(100, metric)
    configure(idx, "auto", "i8", range_slots=SLOTS)
    ids = np.array([7, -1, 40, -7, N_BASE, 999, N_BASE + 5, 0, 2 ** 62, -2 ** 63], dtype=np.int64)
    idx.reset_stats()
    got = idx.search_rows(ids, 5)
    same(got, rows_ref.search_rows(oracle, C, ids, 5, metric))
    bad = [1, 3, 4, 6, 8, 9]
    assert (got[1][bad] == -1).all() and np.isnan(got[0][bad]).all() and (got[1][[0, 2, 5, 7], 0] >= 0).all()
    assert idx.stat("rows_skipped") == len(bad) and idx.stat("rows_queries") == len(ids)
    got = idx.search_range_rows(ids, INF, 5)
    same(got, rows_ref.search_range_rows(oracle, C, ids, INF, 5, metric))
    assert got[2][bad].tolist() == [0] * len(bad) and idx.stat("rows_skipped") == 2 * len(bad)
    # all slots invalid; an empty list of ids
    got = idx.search_rows(np.array([-1, N_BASE]), 3, include_self=True)
    assert (got[1] == -1).all() and np.isnan(got[0]).all()
    d0, r0 = idx.search_rows(np.zeros(0, dtype=np.int64), 3)
    assert d0.shape == r0.shape == (0, 3)


def test_row_offset(bases, oracle):
    idx, C = bases(100, "cosine")
    off = 5000
    configure(idx, "auto", "i8", range_slots=SLOTS, row_offset=off)
    try:
        ids = np.concatenate([draw_ids(33) + off, [40, 4999, off + N_BASE, off]]).astype(np.int64)
        idx.reset_stats()
        got = idx.search_rows(ids, M)
        same(got, rows_ref.search_rows(oracle, C, ids, M, row_offset=off))
        assert (got[1][:33] >= off).all() and (got[1][33:36] == -1).all() and got[1][36, 0] >= off
        assert idx.stat("rows_skipped") == 3
        radius = np.resize(np.array([0.9, INF, 0.8]), len(ids))
        same(idx.search_range_rows(ids, radius, M), rows_ref.search_range_rows(oracle, C, ids, radius, M, row_offset=off))
    finally:
        idx.set_option("row_offset", 0)


def test_argument_errors_change_nothing(pkg, bases):
    idx, C = bases(100, "cosine")
    configure(idx, "auto", "i8", range_slots=SLOTS)
    ids = draw_ids(33)
    before = idx.search_rows(ids, 7)
    before_r = idx.search_range_rows(ids, 0.9, 7)
    lib, h = idx._lib, idx._h
    f64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_double, ctypes.c_int64))
    id4 = np.array([1, 2, 3, 40], dtype=np.int64)
    rad = np.full(4, 0.5)
    od, orow, oc = np.empty((4, 8)), np.empty((4, 8), dtype=np.int64), np.empty(4, dtype=np.int64)
    p = lambda a, t: a.ctypes.data_as(t) if a is not None else None  # noqa: E731

    def topk(ia=id4, B=4, k=5, flags=0, da=od, rwa=orow):
        return lib.mi355dr_search_rows(h, p(ia, i64p), B, k, flags, p(da, f64p), p(rwa, i64p))

    def rng(ia=id4, B=4, ra=rad, m=5, flags=0, da=od, rwa=orow, ca=oc):
        return lib.mi355dr_search_range_rows(h, p(ia, i64p), B, p(ra, f64p), m, flags, p(da, f64p), p(rwa, i64p), p(ca, i64p))

    assert topk() == 0 and rng() == 0 and topk(flags=1) == 0 and rng(flags=1) == 0
    stats = {key: idx.stat(key) for key in ("rows_searches", "rows_queries", "rows_skipped", "range_searches", "passes")}
    assert topk(B=-1) == E_INVALID and topk(k=0) == E_INVALID and topk(k=-2) == E_INVALID
    assert topk(flags=2) == E_INVALID and b"flag" in lib.mi355dr_last_error(h) and topk(flags=3) == E_INVALID
    for null in ("ia", "da", "rwa"):
        assert topk(**{null: None}) == E_INVALID
    assert rng(B=-1) == E_INVALID and rng(m=0) == E_INVALID and rng(m=-3) == E_INVALID and rng(flags=2) == E_INVALID
    assert rng(ra=np.array([0.5, np.nan, 0.5, 0.5])) == E_INVALID and b"NaN" in lib.mi355dr_last_error(h)
    for null in ("ia", "ra", "da", "rwa", "ca"):
        assert rng(**{null: None}) == E_INVALID
    assert {key: idx.stat(key) for key in stats} == stats
    assert topk(B=0) == 0 and rng(B=0) == 0                              # a valid no-op
    with pytest.raises(ValueError):
        idx.search_range_rows(ids, np.nan, 5)
    with pytest.raises(pkg.NativeError) as e:
        idx.search_rows(ids, 0)
    assert e.value.code == E_INVALID
    same(idx.search_rows(ids, 7), before)
    same(idx.search_range_rows(ids, 0.9, 7), before_r)


# ---- 5. internal blocks ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["auto", "scan"])
def test_internal_blocks(bases, ref, oracle, path):
    idx, C = bases(100, "cosine")
    configure(idx, path, "i8", range_slots=SLOTS)
    ids = np.resize(np.arange(N_BASE, dtype=np.int64), 1030)              # splits at 1024; ids cycle over the base
    ids[1027] = -1
    same(idx.search_rows(ids, M), ref("search_rows", C, ("blocks",), ids, M, "cosine"))
    ds, rs = rows_ref.self_masked_sorted(oracle, C, np.where(ids >= 0, ids, 0))
    radius, _ = range_ref.radius_admitting(ds, rs, wanted_counts(1030, M, SLOTS))
    same(idx.search_range_rows(ids, radius, M), ref("search_range_rows", C, ("blocks",), ids, radius, M, "cosine"))


# ---- 6. removed, updated and compacted rows ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["auto", "scan"])
def test_mutations(pkg, oracle, path):
    d = 100
    C = base_rows(d, seed=2).copy()
    ids = np.array([300, 301, 302, 40, 500, 7, 8, 0, 999, 611, 5, 300], dtype=np.int64)
    live = np.ones(N_BASE, dtype=bool)

    def check(idx, C_now, q_ids, live_now):
        for k in (3, M):
            same(idx.search_rows(q_ids, k), rows_ref.search_rows(oracle, C_now, q_ids, k, "cosine", live_now))
        same(idx.search_rows(q_ids, 3, include_self=True), rows_ref.search_rows(oracle, C_now, q_ids, 3, "cosine", live_now, True))
        radius = np.resize(np.array([1e-3, 0.85, INF]), len(q_ids))
        same(idx.search_range_rows(q_ids, radius, 4), rows_ref.search_range_rows(oracle, C_now, q_ids, radius, 4, "cosine", live_now))

    with pkg.Mi355Index(d) as idx:
        idx.add(C)
        configure(idx, path, "i8", range_slots=SLOTS)
        check(idx, C, ids, None)
        idx.remove_rows([40, 500])                                   # rows 300 ... 302 lose a neighbour; 40 is no row any more
        live[[40, 500]] = False
        check(idx, C, ids, live)
        got = idx.search_rows(ids, 3)
        assert got[1][0].tolist()[:2] == [301, 302] and (got[1][3:5] == -1).all() and np.isnan(got[0][3:5]).all()
        idx.reset_stats()
        idx.search_rows(ids, 3)
        assert idx.stat("rows_skipped") == 2
        idx.update_rows([7], C[8:9])                                 # 7 and 8 become each other's nearest
        C[7] = C[8]
        check(idx, C, ids, live)
        got = idx.search_rows(ids, 3)
        assert got[1][5, 0] == 8 and got[1][6, 0] == 7
        new_of_old = idx.compact()
        keep = np.flatnonzero(live)
        assert np.array_equal(new_of_old[keep], np.arange(len(keep))) and (new_of_old[[40, 500]] == -1).all()
        check(idx, np.ascontiguousarray(C[keep]), new_of_old[ids], None)   # the removed rows' ids became -1: blank lines


# ---- 7. views ---------------------------------------------------------------------------------------------------------------------

def test_views_refuse_and_name_the_parent(pkg, bases, oracle):
    idx, C = bases(100, "cosine")
    configure(idx, "auto", "i8", range_slots=SLOTS)
    ids = draw_ids(33)
    with idx.view(row_ids=np.arange(0, 400)) as v:
        buf = v.dev_alloc(4096)
        try:
            calls = (lambda: v.search_rows(ids, 3), lambda: v.search_rows(ids, 3, include_self=True),
                     lambda: v.search_range_rows(ids, 0.5, 3), lambda: v.search_rows_device(ids, 3, buf, buf),
                     lambda: v.search_range_rows_device(ids, 0.5, 3, buf, buf, buf))
            for call in calls:
                with pytest.raises(pkg.NativeError, match="parent") as e:
                    call()
                assert e.value.code == E_INVALID
            assert v.stat("rows_searches") == 0
        finally:
            v.dev_free(buf)
    same(idx.search_rows(ids, 3), rows_ref.search_rows(oracle, C, ids, 3))


# ---- 8. the range form ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", PATHS)
def test_range_counts_around_the_cut(bases, oracle, ref, path, dtype, metric):
    idx, C = bases(100, metric)
    configure(idx, path, dtype, range_slots=SLOTS, cand_cap=2048, range_chunk_rows=1 << 21)
    B = 33
    ids = draw_ids(B)
    ds, rs = rows_ref.self_masked_sorted(oracle, C, ids, metric)
    radius, counts = range_ref.radius_admitting(ds, rs, wanted_counts(B, M, SLOTS))
    if metric == "cosine":
        assert {0, 1, M - 1, M, M + 1} <= set(counts.tolist()) and (counts > SLOTS).any()
        assert ids[0] == 5 and np.isnan(ds[0]).all()                 # the zero row: NaN to itself, never in range
    exp = ref("search_range_rows", C, ("cut", metric), ids, radius, M, metric)
    assert np.array_equal(exp[2], counts)
    got = idx.search_range_rows(ids, radius, M)
    same(got, exp)
    assert not (got[1] == ids[:, None]).any()
    # with the row itself: mi355dr_search_range of the stored vectors
    inc = idx.search_range_rows(ids, radius, M, include_self=True)
    same(inc, ref("search_range_rows", C, ("cut-self", metric), ids, radius, M, metric, None, True))
    same(inc, idx.search_range(np.ascontiguousarray(C[ids]), radius, M))
    assert ((inc[2] - got[2] == 0) | (inc[2] - got[2] == 1)).all()    # the row itself is the whole difference
    # the next double below each radius: that row (and its ties) is out
    below = np.nextafter(radius, -INF)
    same(idx.search_range_rows(ids, below, M), rows_ref.search_range_rows(oracle, C, ids, below, M, metric))


# ---- 9. knn_graph and near_duplicates ---------------------------------------------------------------------------------------------

def test_knn_graph_and_near_duplicates(bases, oracle, ref):
    idx, C = bases(100, "cosine")
    configure(idx, "auto", "i8", range_slots=SLOTS)
    every = np.arange(N_BASE, dtype=np.int64)
    exp = ref("search_rows", C, ("graph",), every, M, "cosine")
    same(idx.knn_graph(M, block=384), exp)                           # blocks of 384, 384 and 232 ids
    same(idx.knn_graph(M), exp)
    part = idx.knn_graph(3, row0=290, row1=310, block=7)
    same(part, rows_ref.search_rows(oracle, C, every[290:310], 3))
    # from the oracle's distances: the copies are within 1e-3 of each other, no other pair of the seeded base is
    nearest = exp[0][:, 0]
    others = np.setdiff1d(every, DUPS)
    radius = 1e-3
    assert (nearest[DUPS] <= radius).all() and not (nearest[others] <= radius).any()
    got = idx.near_duplicates(radius, max_results=5, block=384)
    same(got, rows_ref.search_range_rows(oracle, C, every, radius, 5))
    assert np.flatnonzero(got[2] > 0).tolist() == DUPS and got[2][DUPS].tolist() == [3, 3, 3, 3]
    assert got[1][302, :3].tolist() == [40, 300, 301]


# ---- 10. one larger case on the production screens -------------------------------------------------------------------------------

def test_planted_duplicates_on_the_production_screens(pkg, oracle):
    n, d, k = 20_000, 128, 10
    rng = np.random.default_rng(2010)
    C = rng.standard_normal((n, d)).astype(np.float32)
    sizes = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12]                         # 12 copies: more than k + 1, the row itself can lie behind
    spots = rng.choice(n, size=sum(sizes), replace=False)
    planted, at = [], 0
    for s in sizes:
        group = np.sort(spots[at:at + s])
        C[group] = C[group[0]]
        planted.append(group)
        at += s
    ids = np.concatenate([*planted, rng.integers(0, n, size=256 - sum(sizes))]).astype(np.int64)
    exp = rows_ref.search_rows(oracle, C, ids, k)
    last = planted[-1]
    assert exp[1][len(ids) - (256 - sum(sizes)) - 1].tolist() == last[:k].tolist()      # the 12th copy: ten lower copies
    with pkg.Mi355Index(d) as idx:
        idx.add(C)
        configure(idx, "auto", "i8")
        assert n > 16384                                             # above "small_chunk_rows": the persistent screens run
        idx.reset_stats()
        same(idx.search_rows(ids, k), exp)
        assert idx.stat("screen_launches") > 0 and idx.stat("rows_queries") == 256
        same(idx.search_range_rows(ids, 1e-3, 4), _planted_range(oracle, C, ids))


def _planted_range(oracle, C, ids):
    """the near-duplicate answer at radius 1e-3, max_results 4, from the oracle's nearest 14 rows of every slot (random
    Gaussian rows at d = 128 are nowhere near 1e-3 of each other: checked)"""
    ds, rs = oracle.topk_search(C, np.ascontiguousarray(C[ids]), 14)
    assert (ds[:, 13] > 1e-3).all()                                  # every in-range pair is listed
    rs = np.where(rs == ids[:, None], -1, rs)
    return range_ref.search_range(ds, rs, 1e-3, 4)


# ---- 11. the device forms, stats, and the search around a rows call -------------------------------------------------------------

@pytest.mark.parametrize("path", ["auto", "scan"])
def test_device_forms(bases, oracle, path):
    idx, C = bases(768, "ip")
    configure(idx, path, "i8", range_slots=SLOTS)
    B = 130
    ids = draw_ids(B)
    ds, rs = rows_ref.self_masked_sorted(oracle, C, ids, "ip")
    radius, _ = range_ref.radius_admitting(ds, rs, wanted_counts(B, M, SLOTS))
    od, orr, oc = idx.dev_alloc(B * M * 8), idx.dev_alloc(B * M * 8), idx.dev_alloc(B * 8)
    try:
        gd, gr, gc = np.empty((B, M)), np.empty((B, M), dtype=np.int64), np.empty(B, dtype=np.int64)
        idx.search_rows_device(ids, M, od, orr)                       # stream = NULL: the index's own
        idx.dev_download(od, gd)
        idx.dev_download(orr, gr)
        same((gd, gr), rows_ref.search_rows(oracle, C, ids, M, "ip"))
        idx.search_range_rows_device(ids, radius, M, od, orr, oc)
        idx.dev_download(od, gd)
        idx.dev_download(orr, gr)
        idx.dev_download(oc, gc)
        same((gd, gr, gc), rows_ref.search_range_rows(oracle, C, ids, radius, M, "ip"))
    finally:
        for ptr in (od, orr, oc):
            idx.dev_free(ptr)


def test_stats_and_the_search_around(bases, oracle):
    idx, C = bases(100, "cosine")
    configure(idx, "auto", "i8", range_slots=SLOTS)
    rng = np.random.default_rng(11)
    Q = rng.standard_normal((40, 100)).astype(np.float32)
    before = [idx.search(Q, k) for k in (10, 100)]
    ids = np.concatenate([draw_ids(33), [-1, N_BASE]]).astype(np.int64)
    idx.reset_stats()
    idx.search_rows(ids, M)
    assert (idx.stat("rows_searches"), idx.stat("rows_queries"), idx.stat("rows_skipped")) == (1, 35, 2)
    assert idx.stat("passes") > 0 and idx.stat("range_searches") == 0          # the inner pass is the ordinary search
    for (bd, br), k in zip(before, (10, 100)):
        ad, ar = idx.search(Q, k)
        assert np.array_equal(ar, br) and np.array_equal(ad.view(np.uint64), bd.view(np.uint64))
    got = idx.search_range_rows(ids, 0.9, M)
    assert (idx.stat("rows_searches"), idx.stat("rows_queries"), idx.stat("rows_skipped")) == (2, 70, 4)
    # ... and the range pass: what the pass itself counts moves (its counts include the rows themselves), the call counters of
    # mi355dr_search_range do not
    inc = idx.search_range_rows(ids, 0.9, M, include_self=True)
    assert idx.stat("range_in_range") == 2 * int(inc[2].sum()) >= int(got[2].sum()) > 0
    assert idx.stat("range_searches") == idx.stat("range_queries") == 0
    for (bd, br), k in zip(before, (10, 100)):
        ad, ar = idx.search(Q, k)
        assert np.array_equal(ar, br) and np.array_equal(ad.view(np.uint64), bd.view(np.uint64))
    idx.search_rows(ids[:5], 3, include_self=True)
    assert (idx.stat("rows_searches"), idx.stat("rows_queries"), idx.stat("rows_skipped")) == (4, 110, 6)
    idx.reset_stats()
    assert idx.stat("rows_searches") == idx.stat("rows_queries") == idx.stat("rows_skipped") == 0
