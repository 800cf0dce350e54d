"""GPU: MMR search (mi355dr_search_mmr / _device, mi355dr_mmr_select) against the CPU reference in tests/mmr_ref.py, bit for
bit: rows equal, distance bit patterns equal, NaN positions equal.

The reference restates the definition of include/mi355dr.h ("MMR search") in Python floats over the oracle's `topk_search`,
`cosine_distance` and `dot`.  Corpora: 200 Gaussian centres x 10 near-copies (MMR at lambda = 0.5 leaves the plain top-10 for
every query: tests/test_mmr_host.py), and 2000 Gaussian rows."""

import numpy as np
import pytest

import mmr_ref
from mmr_ref import same

pytestmark = pytest.mark.gpu

LAMBDAS = [0.0, 0.3, 0.5, 1.0]


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


@pytest.mark.parametrize("metric", ["cosine", "ip"])
@pytest.mark.parametrize("d", [128, 100, 50], ids=["d128", "d100-vector-staging", "d50-scalar-staging"])
def test_dims_metrics_lambdas(pkg, oracle, d, metric):
    """rows that are whole 64-column pieces, float4 staging with a partial piece, scalar staging; both metrics; every lambda;
    B = 5 and B = 1; lambda = 1 is `search(k)`, k = 1 is the nearest row, lambda = 0.5 leaves the plain top-k"""
    C, Q = mmr_ref.clustered(d)
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(C)
        plain = idx.search(Q, 10)
        same(plain, oracle.topk_search(C, Q, 10, metric=metric))
        for lam in LAMBDAS:
            got = idx.search_mmr(Q, 10, 32, lam)
            same(got, mmr_ref.search_mmr(oracle, C, Q, 10, 32, lam, metric))
            if lam == 1.0:
                same(got, plain)
            if lam == 0.5:
                assert (got[1] != plain[1]).any(axis=1).all()
        same(idx.search_mmr(Q[2], 10, 32, 0.5), mmr_ref.search_mmr(oracle, C, Q[2:3], 10, 32, 0.5, metric))
        same(idx.search_mmr(Q, 1, 32, 0.0), idx.search(Q, 1))
    Cg, Qg = mmr_ref.gaussian(d)
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(Cg)
        same(idx.search_mmr(Qg, 10, 32, 0.5), mmr_ref.search_mmr(oracle, Cg, Qg, 10, 32, 0.5, metric))


@pytest.fixture(scope="module")
def gauss128(pkg):
    C, Q = mmr_ref.gaussian(128)
    with pkg.Mi355Index(128) as idx:
        idx.add(C)
        yield idx, C, Q


@pytest.mark.parametrize("fetch_k", [1, 31, 64, 65, 100, 257, 1024])
def test_fetch_k_and_k(gauss128, oracle, fetch_k):
    """a partial wave, exactly one wave, a second wave, a second round of the four waves, the cap; k = 1, 10 and fetch_k
    (one query where k = fetch_k is long: 1023 picks over up to 1023 candidates)"""
    idx, C, Q = gauss128
    for k in sorted({1, min(10, fetch_k), fetch_k}):
        q = Q if k <= 100 else Q[:1]
        same(idx.search_mmr(q, k, fetch_k, 0.3), mmr_ref.search_mmr(oracle, C, q, k, fetch_k, 0.3))
    same(idx.search_mmr(Q, min(10, fetch_k), fetch_k, 1.0), idx.search(Q, min(10, fetch_k)))


def test_fewer_live_rows_than_fetch_k(pkg, oracle):
    """removed and updated rows, zero rows (NaN, behind every eligible candidate, never picked), k above what is left: the
    NaN / -1 tail; inner product keeps a zero row as an ordinary candidate"""
    rng = np.random.default_rng(17)
    C = rng.standard_normal((90, 50)).astype(np.float32)
    C[[4, 61]] = 0.0
    for metric in ("cosine", "ip"):
        with pkg.Mi355Index(50, metric) as idx:
            idx.add(C)
            C2 = C.copy()
            C2[[7, 8, 30]] = rng.standard_normal((3, 50)).astype(np.float32)
            C2[9] = C2[10]
            idx.update_rows([7, 8, 30, 9], C2[[7, 8, 30, 9]])
            gone = [0, 5, 33, 34, 89]
            idx.remove_rows(gone)
            live = np.setdiff1d(np.arange(90), gone)
            Q = (C2[[9, 40, 4]] + 0.2 * rng.standard_normal((3, 50))).astype(np.float32)
            for k, fetch_k, lam in ((100, 100, 0.5), (64, 100, 0.0), (10, 100, 0.3), (85, 85, 1.0)):
                d, r = oracle.topk_search(C2[live], Q, fetch_k, metric=metric)
                want = mmr_ref.mmr_from_lists(oracle, C2, d, np.where(r >= 0, live[np.maximum(r, 0)], -1), k, lam, metric)
                got = idx.search_mmr(Q, k, fetch_k, lam)
                same(got, want)
                n_elig = 85 - (2 if metric == "cosine" else 0)
                assert (got[1][:, min(k, n_elig):] == -1).all() and (got[1][:, :min(k, n_elig)] >= 0).all()
                if metric == "cosine":
                    assert not np.isin(got[1], [4, 61]).any()


def test_exact_duplicates(pkg, oracle):
    """three bit-identical rows and a query along them: equal distances (row order decides the candidates' order), pair
    similarity exactly 1 between them"""
    C, Q = mmr_ref.clustered(100)
    C = C.copy()
    C[1500] = C[17]
    C[640] = C[17]
    Q = np.concatenate([C[17:18] * 1.5, Q[:2]])
    with pkg.Mi355Index(100) as idx:
        idx.add(C)
        assert idx.search(Q[:1], 3)[1].tolist() == [[17, 640, 1500]]
        for lam in LAMBDAS:
            same(idx.search_mmr(Q, 12, 40, lam), mmr_ref.search_mmr(oracle, C, Q, 12, 40, lam))
        got = idx.search_mmr(Q[:1], 12, 40, 0.3)[1][0].tolist()
        assert got[0] == 17 and got[1] not in (640, 1500)


def test_row_offset(pkg, oracle):
    C, Q = mmr_ref.clustered(50)
    off = 3_000_000_000
    with pkg.Mi355Index(50) as idx:
        idx.add(C)
        idx.set_option("row_offset", off)
        got = idx.search_mmr(Q, 10, 33, 0.5)
        same(got, mmr_ref.search_mmr(oracle, C, Q, 10, 33, 0.5, row_offset=off))
        assert (got[1] >= off).all()
        pool = np.stack([np.random.default_rng(b).choice(2000, size=40, replace=False) for b in range(len(Q))])
        same(idx.mmr_select(Q, 10, pool + off, 0.5), mmr_ref.mmr_select(oracle, C, Q, 10, pool + off, 0.5, row_offset=off))
        same(idx.mmr_select(Q, 10, pool, 0.5), (np.full((len(Q), 10), np.nan), np.full((len(Q), 10), -1)))   # below row_offset: other shards' rows


def test_two_internal_blocks(pkg, oracle):
    """B = 1030: a block of 1024 queries and one of 6, host and device forms"""
    C, _ = mmr_ref.gaussian(50)
    Q = np.random.default_rng(3).standard_normal((1030, 50)).astype(np.float32)
    with pkg.Mi355Index(50) as idx:
        idx.add(C)
        want = mmr_ref.search_mmr(oracle, C, Q, 5, 16, 0.5)
        same(idx.search_mmr(Q, 5, 16, 0.5), want)
        pq, od, orr = idx.dev_alloc(Q.nbytes), idx.dev_alloc(len(Q) * 5 * 8), idx.dev_alloc(len(Q) * 5 * 8)
        idx.dev_upload(pq, Q)
        idx.search_mmr_device(pq, len(Q), 5, 16, od, orr, 0.5)
        gd, gr = np.empty((len(Q), 5)), np.empty((len(Q), 5), dtype=np.int64)
        idx.dev_download(od, gd)
        idx.dev_download(orr, gr)
        same((gd, gr), want)
        for p in (pq, od, orr):
            idx.dev_free(p)


def test_screened_path(pkg, oracle):
    """N = 70 000, B = 200: the candidates come from the MFMA screens (screen launches counted during the MMR call)"""
    rng = np.random.default_rng(70)
    C = rng.standard_normal((70_000, 128)).astype(np.float32)
    Q = rng.standard_normal((200, 128)).astype(np.float32)
    with pkg.Mi355Index(128) as idx:
        idx.add(C)
        idx.reset_stats()
        got = idx.search_mmr(Q, 10, 32, 0.5)
        assert idx.stat("screen_launches") > 0
        same(got, mmr_ref.search_mmr(oracle, C, Q, 10, 32, 0.5))


def test_device_form_behind_a_block_in_flight(gauss128, oracle):
    """the device form arrives while an async block is in flight: that block is completed first, both results are right, and
    an ordinary search afterwards is unchanged"""
    idx, C, Q = gauss128
    k, fetch_k = 7, 65
    full = oracle.topk_search(C, Q, 33)
    want = mmr_ref.search_mmr(oracle, C, Q, k, fetch_k, 0.5)
    pq, od, orr = idx.dev_alloc(Q.nbytes), idx.dev_alloc(len(Q) * k * 8), idx.dev_alloc(len(Q) * k * 8)
    od2, or2 = idx.dev_alloc(len(Q) * 33 * 8), idx.dev_alloc(len(Q) * 33 * 8)
    idx.dev_upload(pq, Q)
    ticket = idx.search_device_async(pq, len(Q), 33, od2, or2)            # in flight ...
    idx.search_mmr_device(pq, len(Q), k, fetch_k, od, orr, 0.5)           # ... when the MMR call arrives
    gd, gr = np.empty((len(Q), k)), np.empty((len(Q), k), dtype=np.int64)
    idx.dev_download(od, gd)
    idx.dev_download(orr, gr)
    same((gd, gr), want)
    idx.search_wait(ticket)
    gd, gr = np.empty((len(Q), 33)), np.empty((len(Q), 33), dtype=np.int64)
    idx.dev_download(od2, gd)
    idx.dev_download(or2, gr)
    same((gd, gr), full)
    same(idx.search(Q, 33), full)
    for p in (pq, od, orr, od2, or2):
        idx.dev_free(p)


@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_mmr_select(pkg, oracle, metric):
    """each query's own pool: shuffled, with duplicates, -1 padding, ids outside the index and removed rows; a zero row in the
    pool; m = 0; m = 1024; k above the pool; lambda = 1 is `search_subset` over the pool"""
    C, Q = mmr_ref.clustered(100)
    C = C.copy()
    C[123] = 0.0
    rng = np.random.default_rng(23)
    gone = np.array([11, 500, 1999])
    live = np.ones(2000, dtype=bool)
    live[gone] = False
    with pkg.Mi355Index(100, metric) as idx:
        idx.add(C)
        idx.remove_rows(gone)
        near = oracle.topk_search(C, Q, 60, metric=metric)[1]
        pool = np.concatenate([near, near[:, :9], np.tile(gone, (len(Q), 1)),
                               np.tile([-1, -1, 2000, 2**40, -5, 123], (len(Q), 1))], axis=1)
        pool = rng.permuted(pool, axis=1)
        for k, lam in ((10, 0.5), (10, 0.0), (70, 0.3), (1, 0.5)):
            same(idx.mmr_select(Q, k, pool, lam), mmr_ref.mmr_select(oracle, C, Q, k, pool, lam, metric, live=live))
        for b in range(2):
            same(idx.mmr_select(Q[b], 20, pool[b], 1.0), idx.search_subset(Q[b], 20, pool[b]))
        got = idx.mmr_select(Q, 4, np.zeros((len(Q), 0), dtype=np.int64), 0.5)
        assert (got[1] == -1).all() and np.isnan(got[0]).all()
        big = np.stack([rng.permutation(2000)[:1024] for _ in range(2)])
        same(idx.mmr_select(Q[:2], 10, big, 0.5), mmr_ref.mmr_select(oracle, C, Q[:2], 10, big, 0.5, metric, live=live))


def test_refusals(pkg, gauss128):
    from autorag_research_amd._native import NativeError

    idx, C, Q = gauss128
    pool = np.arange(20)[None, :].repeat(len(Q), axis=0)
    INVALID, UNSUPPORTED = -1, -4

    def refused(code, fn, *a):
        with pytest.raises(NativeError) as e:
            fn(*a)
        assert e.value.code == code, (e.value, a)

    import autorag_research_amd._native as nat
    lib = nat.load()
    assert lib.mi355dr_search_mmr(None, None, 0, 1, 1, 0.5, None, None) != 0
    for lam in (-0.01, 1.01, float("nan"), float("inf")):
        refused(INVALID, idx.search_mmr, Q, 5, 10, lam)
        refused(INVALID, idx.mmr_select, Q, 5, pool, lam)
    refused(INVALID, idx.search_mmr, Q, 0, 10, 0.5)
    refused(INVALID, idx.mmr_select, Q, 0, pool, 0.5)
    refused(INVALID, idx.search_mmr, Q, 11, 10, 0.5)
    refused(UNSUPPORTED, idx.search_mmr, Q, 5, 1025, 0.5)
    refused(UNSUPPORTED, idx.mmr_select, Q, 5, np.zeros((len(Q), 1025), dtype=np.int64), 0.5)
    refused(INVALID, idx.search_mmr_device, 0, 3, 5, 10, 0, 0, 0.5)               # null buffers with work to do
    import ctypes
    h, f32p, f64p, i64p = idx._h, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    out_d, out_r = np.empty((len(Q), 5)), np.empty((len(Q), 5), dtype=np.int64)
    qp, dp, rp = Q.ctypes.data_as(f32p), out_d.ctypes.data_as(f64p), out_r.ctypes.data_as(i64p)
    assert lib.mi355dr_mmr_select(h, qp, len(Q), 5, None, 20, 0.5, dp, rp) == INVALID       # a null list with m > 0
    assert lib.mi355dr_mmr_select(h, qp, len(Q), 5, pool.ctypes.data_as(i64p), -1, 0.5, dp, rp) == INVALID
    assert lib.mi355dr_mmr_select(h, None, len(Q), 5, pool.ctypes.data_as(i64p), 20, 0.5, dp, rp) == INVALID
    assert lib.mi355dr_search_mmr(h, qp, len(Q), 5, 10, 0.5, None, rp) == INVALID
    assert lib.mi355dr_search_mmr(h, qp, len(Q), -3, 10, 0.5, dp, rp) == INVALID
    with pytest.raises(ValueError):
        idx.mmr_select(Q, 5, np.zeros((2, 2, 2), np.int64))
    with idx.view(row_ids=np.arange(100)) as v:                                    # a view speaks the parent's ids
        refused(INVALID, v.search_mmr, Q, 5, 10, 0.5)
        refused(INVALID, v.mmr_select, Q, 5, pool, 0.5)
        refused(INVALID, v.search_mmr_device, 0, 3, 5, 10, 0, 0, 0.5)
    same(idx.search_mmr(Q, 5, 10, 0.5), idx.search_mmr(Q, 5, 10, 0.5))             # the handle still serves


def test_stats(gauss128, oracle):
    """mmr_searches counts calls, mmr_queries their queries, mmr_pairs_scored the (picked row, unselected candidate) dots:
    picks - 1 updates over the candidates still unselected, none after the last pick"""
    idx, C, Q = gauss128
    idx.reset_stats()
    assert (idx.stat("mmr_searches"), idx.stat("mmr_queries"), idx.stat("mmr_pairs_scored")) == (0, 0, 0)
    idx.search_mmr(Q, 10, 32, 0.5)
    pairs = len(Q) * sum(32 - t - 1 for t in range(9))
    assert pairs == mmr_ref.search_mmr(oracle, C, Q, 10, 32, 0.5)[2]
    assert (idx.stat("mmr_searches"), idx.stat("mmr_queries"), idx.stat("mmr_pairs_scored")) == (1, len(Q), pairs)
    idx.search_mmr(Q[:2], 1, 32, 0.5)                                              # one pick: nothing scored
    assert (idx.stat("mmr_searches"), idx.stat("mmr_queries"), idx.stat("mmr_pairs_scored")) == (2, len(Q) + 2, pairs)
    pool = np.tile(np.r_[np.arange(12), [-1, 5, 5, 4000]], (3, 1))                 # 12 candidates each
    idx.mmr_select(Q[:3], 12, pool, 0.5)
    pairs += 3 * sum(12 - t - 1 for t in range(11))
    assert (idx.stat("mmr_searches"), idx.stat("mmr_queries"), idx.stat("mmr_pairs_scored")) == (3, len(Q) + 5, pairs)
    assert idx.stat("subset_searches") == 0
    idx.reset_stats()
    assert idx.stat("mmr_pairs_scored") == 0
