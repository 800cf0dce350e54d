"""GPU: search by examples and Rocchio feedback (mi355dr_combine_rows / mi355dr_search_examples / mi355dr_search_feedback and
their Python wrappers) -- queries combined from stored rows on the device, the listed rows struck out of the answer.

Every case compares ALL bits of the combined vectors, ALL B x k distances bit for bit, all rows, the NaN positions and the
stats with tests/examples_ref.py over the oracle's norms and distances."""

import ctypes

import numpy as np
import pytest

import examples_ref as xr
from examples_ref import N_BASE, base_rows, same_lists

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
PATHS = ["auto", "screen", "scan"]
DTYPES = ["i8", "bf16"]
METRICS = ["cosine", "ip"]
STATS = ("examples_searches", "examples_queries", "examples_skipped", "examples_skipped_slots", "feedback_searches")
B_SLOTS = 16


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def configure(idx, path="auto", dtype="i8", **options):
    idx.set_option("path", path)
    idx.set_option("screen_dtype", dtype)
    for key, value in options.items():
        idx.set_option(key, value)


@pytest.fixture(scope="module")
def bases(pkg):
    """(index, C) per (d, metric), built once and shared; every test sets the options it depends on"""
    made = {}

    def get(d, metric):
        if (d, metric) not in made:
            C = base_rows(d)
            idx = pkg.Mi355Index(d, metric)
            idx.add(C)
            made[d, metric] = (idx, C)
        return made[d, metric]

    yield get
    for idx, _ in made.values():
        idx.close()


@pytest.fixture(scope="module")
def ref(oracle):
    """the reference's answers, computed once per case and shared read-only among the paths and screen types"""
    made = {}

    def get(kind, key, *args, **kw):
        if (kind, key) not in made:
            made[kind, key] = getattr(xr, kind)(oracle, *args, **kw)
            for a in made[kind, key]:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        return made[kind, key]

    return get


def make_slots(mp, mn, d, with_base, seed=0, off=0):
    """B_SLOTS slots: random live rows, then one slot per way an example or a base can be invalid.  -> (Q or None, pos, neg)"""
    rng = np.random.default_rng(100 * mp + 10 * mn + seed)
    pos = rng.integers(20, N_BASE, size=(B_SLOTS, mp)).astype(np.int64)
    neg = rng.integers(20, N_BASE, size=(B_SLOTS, mn)).astype(np.int64)
    pos[0, -1] = -1                                      # padding
    pos[1, 0], pos[2, 0], pos[3, 0], pos[4, 0] = 5, 17, 18, 19    # the zero / NaN / inf / 1e20 rows: skipped
    pos[5, 0], pos[6, 0] = N_BASE + 7, -5                # outside the shard
    pos[7, :] = -1                                       # only invalid examples
    pos[7, 0] = 5
    neg[7, :] = 17
    if mp >= 3:
        pos[8, 1] = pos[8, 0]                            # a row listed twice: counted twice
        pos[9, :3] = [40, 300, 7]                        # two copies of one vector
    pos[13, 0], pos[14, 0] = 2 ** 62, -2 ** 63
    valid_id = (pos >= 0) & (pos < N_BASE)
    pos, neg = np.where(valid_id, pos + off, pos), neg + off
    Q = None
    if with_base:
        Q = rng.standard_normal((B_SLOTS, d)).astype(np.float32)
        Q[10] = 0.0                                      # invalid bases: zero, NaN, a norm that overflows
        Q[11, 3] = np.nan
        Q[12] *= 1e20
    return Q, pos, neg


def stats_of(idx):
    return {key: idx.stat(key) for key in STATS}


def check_combine(idx, oracle, C, Q, pos, neg, alpha, beta, gamma, metric, off=0, live=None):
    idx.reset_stats()
    vec, valid = idx.combine_rows(pos, neg if neg.shape[1] else None, Q, alpha, beta, gamma)
    ev, evalid, st = xr.combine(oracle, C, Q, pos, neg, alpha, beta, gamma, metric, off, live)
    assert np.array_equal(valid, evalid)
    assert np.array_equal(vec.view(np.uint32), ev.view(np.uint32)), np.flatnonzero((vec.view(np.uint32) != ev.view(np.uint32)).any(axis=1))
    assert stats_of(idx) == {"examples_searches": 1, "examples_queries": len(pos), "examples_skipped": st["skipped"],
                             "examples_skipped_slots": st["skipped_slots"], "feedback_searches": 0}
    return vec, valid, st


# ---- 1. the combination alone ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("mn", [0, 2])
@pytest.mark.parametrize("mp", [1, 3, 64])
@pytest.mark.parametrize("d", [70, 768])
@pytest.mark.parametrize("metric", METRICS)
def test_combine_rows(bases, oracle, metric, d, mp, mn, with_base):
    idx, C = bases(d, metric)
    Q, pos, neg = make_slots(mp, mn, d, with_base)
    _, valid, st = check_combine(idx, oracle, C, Q, pos, neg, 0.6, 1.0, 0.5, metric)
    assert st["skipped"] >= 8 + mn and valid[7] == (1 if with_base else 0)
    assert valid[10:13].tolist() == ([0, 0, 0] if with_base else [1, 1, 1])
    assert valid[1] == (1 if with_base or mp > 1 or mn else 0)          # its only positive is the zero row


@pytest.mark.parametrize("metric", METRICS)
def test_combine_weights_and_cancellation(bases, oracle, metric):
    idx, C = bases(70, metric)
    Q, pos, neg = make_slots(3, 2, 70, True, seed=1)
    check_combine(idx, oracle, C, Q, pos, neg, 0.0, 1.0, 1.0, metric)               # alpha = 0: the base only decides validity
    check_combine(idx, oracle, C, Q, pos, neg, 1.0, 0.0, 0.0, metric)
    check_combine(idx, oracle, C, Q, pos, neg, 1e-3, 7.5, 1e3, metric)
    # beta = gamma on the same row, and on a copy of it: exactly +0.0 everywhere, the slot valid
    one = np.array([[123], [40], [302]], dtype=np.int64)
    vec, valid, _ = check_combine(idx, oracle, C, None, one, np.array([[123], [300], [302]], dtype=np.int64), 1.0, 2.0, 2.0, metric)
    assert not vec.view(np.uint32).any() and valid.tolist() == [1, 1, 1]
    # a weight that overflows fp32: the vector is what the arithmetic gives (inner product: no normalisation)
    if metric == "ip":
        vec, valid, _ = check_combine(idx, oracle, C, Q[:3] * np.float32(1e8), pos[:3], neg[:3], 1e35, 1.0, 1.0, metric)
        assert np.isinf(vec).any() and valid.tolist() == [1, 1, 1]
    # ragged Python lists are padded with -1; a centroid
    vec, valid = idx.combine_rows([[1, 2, 3], [4], []], None, None)
    ev, evalid, _ = xr.combine(oracle, C, None, [[1, 2, 3], [4], []], None, 1.0, 1.0, 1.0, metric)
    assert np.array_equal(vec.view(np.uint32), ev.view(np.uint32)) and valid.tolist() == evalid.tolist() == [1, 1, 0]
    v0, ok0 = idx.combine_rows(np.zeros((0, 3), dtype=np.int64))
    assert v0.shape == (0, 70) and ok0.shape == (0,)


def test_combine_row_offset_and_device_form(bases, oracle):
    idx, C = bases(768, "cosine")
    off = 5000
    idx.set_option("row_offset", off)
    try:
        Q, pos, neg = make_slots(3, 2, 768, True, seed=2, off=off)
        pos[15, 0], pos[15, 1] = 40, off + N_BASE            # below the offset and one past the end: no rows of the index
        check_combine(idx, oracle, C, Q, pos, neg, 1.0, 1.0, 1.0, "cosine", off)
    finally:
        idx.set_option("row_offset", 0)
    Q, pos, neg = make_slots(64, 2, 768, True, seed=3)
    exp = xr.combine(oracle, C, Q, pos, neg, 0.5, 1.0, 0.25, "cosine")
    for base in (Q, None):
        if base is None:
            exp = xr.combine(oracle, C, None, pos, neg, 0.5, 1.0, 0.25, "cosine")
        qp = idx.dev_alloc(Q.nbytes)
        ov, ok = idx.dev_alloc(Q.nbytes), idx.dev_alloc(4 * B_SLOTS)
        try:
            idx.dev_upload(qp, Q)
            idx.reset_stats()
            idx.combine_rows_device(pos, neg, qp if base is not None else None, ov, ok, 0.5, 1.0, 0.25)
            vec, valid = np.empty_like(Q), np.empty(B_SLOTS, dtype=np.int32)
            idx.dev_download(ov, vec)
            idx.dev_download(ok, valid)
        finally:
            for p in (qp, ov, ok):
                idx.dev_free(p)
        assert np.array_equal(vec.view(np.uint32), exp[0].view(np.uint32)) and np.array_equal(valid, exp[1])
        assert idx.stat("examples_skipped") == exp[2]["skipped"] and idx.stat("examples_skipped_slots") == exp[2]["skipped_slots"]


# ---- 2. search by examples ---------------------------------------------------------------------------------------------------------

def search_slots(d, with_base):
    Q, pos, neg = make_slots(3, 2, d, with_base, seed=4)
    pos[15] = [40, -1, -1]                                   # a row with three copies: they stay in the answer
    neg[15] = [700, 701]
    return Q, pos, neg


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", PATHS)
def test_search_examples(bases, ref, path, dtype, metric, with_base):
    d = 70
    idx, C = bases(d, metric)
    configure(idx, path, dtype, cand_cap=2048)
    Q, pos, neg = search_slots(d, with_base)
    for k in (1, 10, 32):
        for keep in (False, True):
            exp = ref("search_examples", (metric, with_base, k, keep), C, Q, pos, neg, 0.8, 1.0, 0.5, k, metric, keep=keep)
            idx.reset_stats()
            got = idx.search_examples(pos, k, neg, Q, 0.8, 1.0, 0.5, keep=keep)
            same_lists(got, exp)
            assert stats_of(idx) == {"examples_searches": 1, "examples_queries": B_SLOTS, "examples_skipped": exp[2]["skipped"],
                                     "examples_skipped_slots": exp[2]["skipped_slots"], "feedback_searches": 0}
            listed = np.concatenate([pos, neg], axis=1)
            for b in range(B_SLOTS):
                hit = np.isin(got[1][b][got[1][b] >= 0], listed[b]).any()
                assert not hit or keep
    if not with_base and metric == "cosine":                 # q' is the unit vector of row 40: its copies first, itself struck
        assert idx.search_examples(pos, 10, neg)[1][15, :3].tolist() == [300, 301, 302]
        assert idx.search_examples(pos, 10, neg, keep=True)[1][15, :4].tolist() == [40, 300, 301, 302]


def test_search_examples_d768_and_the_device_form(bases, ref):
    d = 768
    idx, C = bases(d, "cosine")
    configure(idx, "auto", "i8", cand_cap=2048)
    Q, pos, neg = search_slots(d, True)
    k = 10
    exp = ref("search_examples", ("d768",), C, Q, pos, neg, 1.0, 1.0, 1.0, k, "cosine")
    same_lists(idx.search_examples(pos, k, neg, Q), exp)
    qp, od, orr = idx.dev_alloc(Q.nbytes), idx.dev_alloc(B_SLOTS * k * 8), idx.dev_alloc(B_SLOTS * k * 8)
    try:
        idx.dev_upload(qp, Q)
        idx.search_examples_device(pos, neg, qp, k, od, orr)         # stream = NULL: the index's own
        gd, gr = np.empty((B_SLOTS, k)), np.empty((B_SLOTS, k), dtype=np.int64)
        idx.dev_download(od, gd)
        idx.dev_download(orr, gr)
        same_lists((gd, gr), exp)
        idx.search_examples_device(pos, neg, None, k, od, orr, keep=True)
        idx.dev_download(od, gd)
        idx.dev_download(orr, gr)
        same_lists((gd, gr), ref("search_examples", ("d768", "nobase"), C, None, pos, neg, 1.0, 1.0, 1.0, k, "cosine", keep=True))
    finally:
        for p in (qp, od, orr):
            idx.dev_free(p)


def test_depth_1024_is_the_limit(pkg, bases, ref):
    idx, C = bases(70, "cosine")
    configure(idx, "auto", "i8", cand_cap=2048)
    rng = np.random.default_rng(9)
    pos = rng.integers(20, N_BASE, size=(3, 62)).astype(np.int64)
    neg = rng.integers(20, N_BASE, size=(3, 2)).astype(np.int64)
    exp = ref("search_examples", ("depth",), C, None, pos, neg, 1.0, 1.0, 1.0, 960, "cosine")
    got = idx.search_examples(pos, 960, neg)                         # k + mp + mn = 1024: accepted
    same_lists(got, exp)
    assert (got[1][:, 0] >= 0).all() and (got[1][:, 959] == -1).all()     # fewer live rows than k: the NaN / -1 tail
    before = stats_of(idx)
    with pytest.raises(pkg.NativeError) as e:
        idx.search_examples(pos, 961, neg)                           # 1025
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(pkg.NativeError) as e:
        idx.search_examples(pos, 1025, neg, keep=True)
    assert e.value.code == E_UNSUPPORTED
    assert stats_of(idx) == before
    same_lists(idx.search_examples(pos, 1024, neg, keep=True),
               ref("search_examples", ("depth", "keep"), C, None, pos, neg, 1.0, 1.0, 1.0, 1024, "cosine", keep=True))


def test_internal_blocks(bases, ref):
    idx, C = bases(70, "cosine")
    configure(idx, "auto", "i8", cand_cap=2048)
    B = 1025                                                         # splits at 1024
    rng = np.random.default_rng(10)
    pos = rng.integers(0, N_BASE, size=(B, 2)).astype(np.int64)
    neg = rng.integers(0, N_BASE, size=(B, 1)).astype(np.int64)
    pos[1023], pos[1024, 1] = -1, -1
    Q = rng.standard_normal((B, 70)).astype(np.float32)
    Q[1022] = 0.0
    exp = ref("search_examples", ("blocks",), C, Q, pos, neg, 1.0, 1.0, 1.0, 5, "cosine")
    idx.reset_stats()
    got = idx.search_examples(pos, 5, neg, Q)
    same_lists(got, exp)
    assert idx.stat("examples_skipped") == exp[2]["skipped"] and idx.stat("examples_skipped_slots") == exp[2]["skipped_slots"] >= 1
    assert (got[1][1022] == -1).all() and (got[1][1024] >= 0).all()


@pytest.mark.parametrize("path", ["auto", "scan"])
def test_mutations(pkg, oracle, path):
    d = 70
    C = base_rows(d, seed=2).copy()
    pos = np.array([[300, 301, 7], [40, 500, -1], [500, -1, -1], [8, 9, 10], [611, 0, 999]], dtype=np.int64)
    neg = np.array([[40], [3], [40], [500], [1]], dtype=np.int64)
    rng = np.random.default_rng(12)
    Q = rng.standard_normal((5, d)).astype(np.float32)
    live = np.ones(N_BASE, dtype=bool)

    def check(idx, C_now, p, n, live_now):
        for base in (None, Q):
            for k in (3, 10):
                idx.reset_stats()
                got = idx.search_examples(p, k, n, base)
                exp = xr.search_examples(oracle, C_now, base, p, n, 1.0, 1.0, 1.0, k, "cosine", 0, live_now)
                same_lists(got, exp)
                assert idx.stat("examples_skipped") == exp[2]["skipped"]
                assert idx.stat("examples_skipped_slots") == exp[2]["skipped_slots"]
        vec, valid = idx.combine_rows(p, n, Q)
        ev, evalid, _ = xr.combine(oracle, C_now, Q, p, n, 1.0, 1.0, 1.0, "cosine", 0, live_now)
        assert np.array_equal(vec.view(np.uint32), ev.view(np.uint32)) and np.array_equal(valid, evalid)
        same_lists(idx.search_feedback(Q, 5, 7), xr.search_feedback(oracle, C_now, Q, 5, 7, 1.0, 0.75, "cosine", 0, live_now))

    with pkg.Mi355Index(d) as idx:
        idx.add(C)
        configure(idx, path, "i8")
        check(idx, C, pos, neg, None)
        idx.remove_rows([40, 500])                                   # removed rows are no examples; they are struck all the same
        live[[40, 500]] = False
        check(idx, C, pos, neg, live)
        got = idx.search_examples(pos, 3, neg)
        assert (got[1][2] == -1).all() and np.isnan(got[0][2]).all()          # its only examples are removed rows
        assert not np.isin(got[1], [40, 500]).any()
        new_of_old = idx.compact()
        keep = np.flatnonzero(live)
        remap = lambda a: np.where(a >= 0, new_of_old[np.maximum(a, 0)], -1)  # noqa: E731
        check(idx, np.ascontiguousarray(C[keep]), remap(pos), remap(neg), None)


def test_empty_index(pkg, oracle):
    rng = np.random.default_rng(13)
    Q = rng.standard_normal((3, 70)).astype(np.float32)
    pos = np.array([[0, 1], [2, -1], [5, 5]], dtype=np.int64)
    with pkg.Mi355Index(70) as idx:
        for base in (None, Q):
            d, r = idx.search_examples(pos, 4, None, base)
            assert d.shape == r.shape == (3, 4) and (r == -1).all() and np.isnan(d).all()
            vec, valid = idx.combine_rows(pos, None, base)
            assert valid.tolist() == ([1, 1, 1] if base is not None else [0, 0, 0])
            ev = xr.combine(oracle, np.zeros((0, 70), np.float32), base, pos, None, 1.0, 1.0, 1.0)[0]
            assert np.array_equal(vec.view(np.uint32), ev.view(np.uint32))
        d, r = idx.search_feedback(Q, 4, 6)
        assert (r == -1).all() and np.isnan(d).all()
        assert idx.stat("examples_skipped") == 4 * 6 and idx.stat("examples_skipped_slots") == 2 * 3 and idx.stat("feedback_searches") == 1


def test_views_refuse_and_name_the_parent(pkg, bases):
    idx, C = bases(70, "cosine")
    Q, pos, neg = search_slots(70, True)
    with idx.view(row_ids=np.arange(0, 400)) as v:
        buf = v.dev_alloc(B_SLOTS * 70 * 8)
        try:
            calls = (lambda: v.combine_rows(pos, neg, Q), lambda: v.search_examples(pos, 3, neg, Q),
                     lambda: v.search_feedback(Q, 3, 5), lambda: v.combine_rows_device(pos, neg, None, buf, buf),
                     lambda: v.search_examples_device(pos, neg, None, 3, buf, buf),
                     lambda: v.search_feedback_device(buf, B_SLOTS, 3, 5, buf, buf))
            for call in calls:
                with pytest.raises(pkg.NativeError, match="parent") as e:
                    call()
                assert e.value.code == E_INVALID
            assert v.stat("examples_searches") == 0
        finally:
            v.dev_free(buf)


def test_argument_errors_change_nothing(pkg, bases):
    idx, C = bases(70, "cosine")
    configure(idx, "auto", "i8")
    Q, pos, neg = search_slots(70, True)
    before = idx.search_examples(pos, 7, neg, Q)
    lib, h = idx._lib, idx._h
    f32p, f64p, i64p, i32p = (ctypes.POINTER(t) for t in (ctypes.c_float, ctypes.c_double, ctypes.c_int64, ctypes.c_int32))
    q4 = np.ascontiguousarray(Q[:4])
    p4, n4 = np.ascontiguousarray(pos[:4]), np.ascontiguousarray(neg[:4])
    od, orow = np.empty((4, 8)), np.empty((4, 8), dtype=np.int64)
    ov, ok = np.empty((4, 70), dtype=np.float32), np.empty(4, dtype=np.int32)
    p = lambda a, t: a.ctypes.data_as(t) if a is not None else None  # noqa: E731

    def search(qa=q4, B=4, pa=p4, mp=3, na=n4, mn=2, al=1.0, be=1.0, ga=1.0, k=5, flags=0, da=od, rwa=orow):
        return lib.mi355dr_search_examples(h, p(qa, f32p), B, p(pa, i64p), mp, p(na, i64p), mn, al, be, ga, k, flags, p(da, f64p),
                                           p(rwa, i64p))

    def combine(qa=q4, B=4, pa=p4, mp=3, na=n4, mn=2, al=1.0, be=1.0, ga=1.0, va=ov, oa=ok):
        return lib.mi355dr_combine_rows(h, p(qa, f32p), B, p(pa, i64p), mp, p(na, i64p), mn, al, be, ga, p(va, f32p), p(oa, i32p))

    def feedback(qa=q4, B=4, k=5, fb_k=6, al=1.0, be=0.75, da=od, rwa=orow):
        return lib.mi355dr_search_feedback(h, p(qa, f32p), B, k, fb_k, al, be, p(da, f64p), p(rwa, i64p))

    assert search() == 0 and combine() == 0 and feedback() == 0 and search(flags=1) == 0 and search(qa=None) == 0
    assert search(na=None, mn=0) == 0 and search(pa=None, mp=0) == 0            # no negatives; a base and no positives
    stats = {key: idx.stat(key) for key in STATS + ("passes",)}
    for call in (search, combine, feedback):
        assert call(B=-1) == E_INVALID
        for w in (np.nan, np.inf, -1.0, -np.inf):
            assert call(al=w) == E_INVALID and call(be=w) == E_INVALID
        assert call(qa=None, **({} if call is feedback else {"pa": None, "mp": 0})) == E_INVALID
    for call in (search, combine):
        assert call(mp=-1) == E_INVALID and call(mn=-1) == E_INVALID and call(ga=np.nan) == E_INVALID and call(ga=-0.5) == E_INVALID
        assert call(pa=None) == E_INVALID and call(na=None) == E_INVALID
    assert search(k=0) == E_INVALID and search(k=-2) == E_INVALID and feedback(k=0) == E_INVALID
    assert feedback(fb_k=0) == E_INVALID and feedback(fb_k=-1) == E_INVALID
    assert search(flags=2) == E_INVALID and b"flag" in lib.mi355dr_last_error(h) and search(flags=3) == E_INVALID
    for null in ("da", "rwa"):
        assert search(**{null: None}) == E_INVALID and feedback(**{null: None}) == E_INVALID
    for null in ("va", "oa"):
        assert combine(**{null: None}) == E_INVALID
    assert feedback(fb_k=1025) == E_UNSUPPORTED and feedback(k=1025) == E_UNSUPPORTED and search(k=1020) == E_UNSUPPORTED
    assert {key: idx.stat(key) for key in stats} == stats
    assert search(B=0) == 0 and combine(B=0) == 0 and feedback(B=0) == 0        # a valid no-op
    same_lists(idx.search_examples(pos, 7, neg, Q), before)


# ---- 3. feedback -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def feedback_indexes(pkg):
    made = {}

    def get(name):
        if name not in made:
            C, Q, metric, k, fb_k, alpha, beta = xr.feedback_case(name)
            idx = pkg.Mi355Index(C.shape[1], metric)
            idx.add(C)
            made[name] = (idx, C, Q, metric, k, fb_k, alpha, beta)
        return made[name]

    yield get
    for entry in made.values():
        entry[0].close()


@pytest.mark.parametrize("path", ["auto", "scan"])
@pytest.mark.parametrize("name", [c[0] for c in xr.FEEDBACK_CASES])
def test_search_feedback(feedback_indexes, ref, name, path):
    idx, C, Q, metric, k, fb_k, alpha, beta = feedback_indexes(name)
    configure(idx, path, "i8", cand_cap=2048)
    exp = ref("search_feedback", (name,), C, Q, k, fb_k, alpha, beta, metric)
    idx.reset_stats()
    got = idx.search_feedback(Q, k, fb_k, alpha, beta)
    same_lists(got, exp)
    assert stats_of(idx) == {"examples_searches": 1, "examples_queries": len(Q), "examples_skipped": 0,
                             "examples_skipped_slots": 0, "feedback_searches": 1}
    assert (got[1] != idx.search(Q, k)[1]).any()                     # the case moves some list (checked on the CPU as well)
    # by construction: the search at fb_k, then the search by examples with those rows and KEEP
    d1, r1 = idx.search(Q, fb_k)
    two = idx.search_examples(np.where(np.isnan(d1), -1, r1), k, None, Q, alpha, beta, 0.0, keep=True)
    same_lists(two, got)
    if name == "short":
        assert (r1[:, len(C):] == -1).all() and (r1[:, len(C) - 1] >= 0).all()     # fewer positives than fb_k
    # the device form
    qp, od, orr = idx.dev_alloc(Q.nbytes), idx.dev_alloc(len(Q) * k * 8), idx.dev_alloc(len(Q) * k * 8)
    try:
        idx.dev_upload(qp, Q)
        idx.search_feedback_device(qp, len(Q), k, fb_k, od, orr, alpha, beta)
        gd, gr = np.empty((len(Q), k)), np.empty((len(Q), k), dtype=np.int64)
        idx.dev_download(od, gd)
        idx.dev_download(orr, gr)
        same_lists((gd, gr), exp)
    finally:
        for p in (qp, od, orr):
            idx.dev_free(p)


@pytest.mark.parametrize("metric", METRICS)
def test_feedback_over_every_row_class(bases, oracle, metric):
    """the base corpus: under inner product the 1e20 row leads every list and is no valid positive (its norm overflows);
    zero and NaN queries are invalid bases"""
    idx, C = bases(70, metric)
    configure(idx, "auto", "i8", cand_cap=2048)
    rng = np.random.default_rng(14)
    Q = rng.standard_normal((9, 70)).astype(np.float32)
    Q[3] = 0.0
    Q[4, 1] = np.nan
    exp = xr.search_feedback(oracle, C, Q, 10, 12, 1.0, 0.75, metric)
    idx.reset_stats()
    same_lists(idx.search_feedback(Q, 10, 12), exp)
    assert idx.stat("examples_skipped") == exp[2]["skipped"] and idx.stat("examples_skipped_slots") == exp[2]["skipped_slots"] == 2
    if metric == "ip":
        assert exp[2]["skipped"] >= 1


# ---- 4. the service and the pipeline -------------------------------------------------------------------------------------------------

def test_service_and_pipeline(pkg):
    from autorag_research_amd import service
    from autorag_research_amd.feedback import Mi355FeedbackRetrievalPipeline
    from helpers import build_golden_stores

    store, g = build_golden_stores()
    ids = list(g["ids"])
    s = service.Mi355RetrievalService(lambda: store)
    try:
        ix = s._unit("chunk").ensure_single()
        emb = [float(x) for x in g["Q"][0]]
        out = s.similar_to_examples([ids[4], ids[9]], [ids[30]], top_k=6, embedding=emb, alpha=0.5, beta=1.0, gamma=0.25)
        d, r = ix.search_examples([[4, 9]], 6, [[30]], g["Q"][:1], 0.5, 1.0, 0.25)
        assert [x["doc_id"] for x in out] == [ids[i] for i in r[0]] and [x["score"] for x in out] == (1.0 - d[0]).tolist()
        assert not {ids[4], ids[9], ids[30]} & {x["doc_id"] for x in out} and all(x["content"] is not None for x in out)
        kept = s.similar_to_examples([ids[4]], top_k=3, keep=True)
        assert kept[0]["doc_id"] == ids[4]
        qids = [f"q{i}" for i in range(6)]
        got = s.vector_search_feedback(qids, top_k=5, fb_k=7, alpha=1.0, beta=0.5)
        d, r = ix.search_feedback(g["Q"], 5, 7, 1.0, 0.5)
        assert [[x["doc_id"] for x in res] for res in got] == [[ids[i] for i in row] for row in r]
        assert [[x["score"] for x in res] for res in got] == (1.0 - d).tolist()
        assert s.vector_search_feedback_by_embedding(emb, top_k=5, fb_k=7, beta=0.5) == got[0]
        # the host composition of the same calls
        d1, r1 = ix.search(g["Q"], 7)
        d2, r2 = ix.search(ix.combine_rows(r1, None, g["Q"], 1.0, 0.5)[0], 5)
        assert np.array_equal(r2, r) and np.array_equal(d2.view(np.uint64), d.view(np.uint64))
    finally:
        s.close()
    p = Mi355FeedbackRetrievalPipeline(lambda: store, "fb", fb_k=7, beta=0.5)
    try:
        stats = p.run(top_k=5, batch_size=4)
        assert stats["failed_queries"] == ["q_noemb"] and stats["total_queries"] == 6 and stats["total_results"] == 30
        for qid, res in zip(qids, got):
            assert store.chunk_results[(p.pipeline_id, qid)] == [(x["doc_id"], x["score"]) for x in res]
    finally:
        p.close()
