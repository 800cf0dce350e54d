"""GPU: the guaranteed exact scan under the AUTO path -- corpora with more than kIrrCap (1024) irregular rows, where no
screen can rank the queries and every query of the block goes to run_scan.  Ids and float8 distances against the CPU
oracle, bit for bit (NaN positions must match, NaN payloads are not part of the contract).

The corpora are sized so that the default chunk ladder of the scan (1024 rows, then x63) meets a second chunk larger than
the candidate list: on rows sorted by rising similarity every row enters the running top-k, that chunk overflows and is
re-run in list-sized pieces.  At 33 <= k <= 128 those pieces once ran with the two-wave prune's 4096-entry stride while the
exact prune sorts at most 4096 entries (k kept + the piece): a piece that did not fit was dropped without a flag."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, B = 29_696, 128, 24   # N - 1024 = 7 x 4096: the re-run pieces behind the first chunk end with the corpus
KS = [32, 33, 64, 100, 128, 129, 1024]       # one-wave / two-wave / general prune edges, and kKMax
ORDERS = ["ascending", "descending", "ties", "gauss"]
N_IRR = 1100                                 # > kIrrCap: no screen on AUTO


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def _same(a, b):
    """two (dist, rows) results agree bit for bit (NaN positions, not payloads)"""
    (da, ra), (db, rb) = a, b
    assert np.array_equal(ra, rb)
    assert np.array_equal(np.isnan(da), np.isnan(db))
    ok = ~np.isnan(da)
    assert np.array_equal(da[ok].view(np.uint64), db[ok].view(np.uint64))


def _check(idx, oracle, C, Q, k, metric="cosine"):
    got = idx.search(Q, k)
    _same(got, oracle.topk_search(C, Q, k, metric=metric))
    return got


def _score(C, q, metric):
    s = C.astype(np.float64) @ q.astype(np.float64)
    return s / np.linalg.norm(C.astype(np.float64), axis=1) if metric == "cosine" else s


def make_case(order, irregular, n=N, d=D, metric="cosine", n_irr=N_IRR, n_loose=0, seed=0):
    """corpus [n, d] and queries [B, d].  The queries share the direction q0: q0 itself, 3 q0, q0 plus noise of four sizes,
    -q0 (the reversed order), and random queries.  `ascending` / `descending` sort the rows by their similarity to q0;
    `ties` makes a third of the rows copies of 50 rows near q0; `gauss` keeps the rows as drawn.  Then the first `n_irr`
    rows are overwritten by irregular ones -- all zero (`zero`), or cycling through 0, NaN and +-inf with ten rows each of
    1e-25, 1e25 and -1e25 among them (`mixed`; those rows have finite distances, 0 and 1: a few of them, fewer than k, or
    they would set every threshold) -- and `n_loose` regular rows get one outlier component (outside the int8 residual limit).  The scan's
    first chunk then holds irregular rows only (its threshold admits every row after it), and the rows behind it, where the
    re-run pieces fall, are regular."""
    rng = np.random.default_rng([seed, d, n, n_irr, n_loose, ORDERS.index(order), int(metric == "ip")])
    q0 = rng.standard_normal(d).astype(np.float32)
    C = rng.standard_normal((n, d)).astype(np.float32)
    if order in ("ascending", "descending"):
        C = C[np.argsort(_score(C, q0, metric), kind="stable")]
        if order == "descending":
            C = C[::-1].copy()
    elif order == "ties":
        base = rng.standard_normal((50, d)).astype(np.float32) + 2.0 * q0[None, :]
        pos = rng.choice(n, size=n // 3, replace=False)
        C[pos] = base[rng.integers(0, 50, size=pos.size)]
    Q = rng.standard_normal((B, d)).astype(np.float32)
    Q[0], Q[1], Q[6] = q0, 3.0 * q0, -q0
    for i, eps in enumerate((1e-3, 1e-2, 5e-2, 0.2)):
        Q[2 + i] = q0 + eps * rng.standard_normal(d).astype(np.float32)
    irr = np.arange(n_irr)
    values = (0.0,) if irregular == "zero" else (0.0, np.nan, np.inf, -np.inf)
    for i, r in enumerate(irr):
        C[r] = values[i % len(values)]
    if irregular == "mixed":
        for j, v in enumerate((1e-25, 1e25, -1e25)):
            C[irr[5 + j:n_irr:n_irr // 10][:10]] = v
    loose = rng.choice(np.arange(n_irr, n), size=n_loose, replace=False)
    C[loose, rng.integers(0, d, size=loose.size)] += 40.0
    return C, Q


_CASES = {}


def case(*args, **kw):
    key = (args, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = make_case(*args, **kw)
    return _CASES[key]


def _assert_unscreened(idx, nq):
    assert idx.stat("irregular_rows") > 1024
    assert idx.stat("screen_launches") == 0
    assert idx.stat("fallback_queries") == nq


@pytest.mark.parametrize("screen", ["auto", "bf16"])
@pytest.mark.parametrize("irregular", ["zero", "mixed"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("k", KS)
def test_auto_without_screen_matches_oracle(pkg, oracle, k, order, irregular, screen):
    """AUTO with more than 1024 irregular rows: no screen runs, every query takes the exact scan, whose overflowed chunk is
    re-run in list-sized pieces (ascending: every row enters the top-k) -- at every prune form's k."""
    C, Q = case(order, irregular)
    with pkg.Mi355Index(D) as idx:
        idx.set_option("screen_dtype", screen)
        idx.add(C)
        _check(idx, oracle, C, Q, k)
        _assert_unscreened(idx, B)


@pytest.mark.parametrize("k,metric", [(33, "cosine"), (100, "cosine"), (129, "cosine"), (1024, "cosine"), (33, "ip"),
                                      (100, "ip")])
@pytest.mark.parametrize("d,scan_dma", [(128, 1), (128, 0), (100, 1)], ids=["k_scan32", "k_scan-d128", "k_scan-d100"])
def test_both_scan_kernels(pkg, oracle, d, scan_dma, k, metric):
    """the LDS-DMA scan (d a multiple of 32), the same d through k_scan (scan_dma = 0), and k_scan at d = 100; cosine and
    inner product, rows sorted by rising score of the queries' shared direction"""
    n = 37_888
    C, Q = case("ascending", "mixed", n=n, d=d, metric=metric)
    with pkg.Mi355Index(d, metric) as idx:
        idx.set_option("scan_dma", scan_dma)
        idx.add(C)
        _check(idx, oracle, C, Q, k, metric)
        _assert_unscreened(idx, B)


@pytest.mark.parametrize("order", ["ascending", "ties"])
@pytest.mark.parametrize("k", KS)
def test_every_route_to_the_scan_agrees(pkg, oracle, k, order):
    """path = scan, AUTO without a screen, and AUTO without a screen at an explicit cand_cap = 2048 return the same bits:
    an unscreened AUTO pass uses the exact path's list stride whatever k is"""
    C, Q = case(order, "mixed")
    res = []
    for opts in ({"path": "scan"}, {}, {"cand_cap": 2048}):
        with pkg.Mi355Index(D) as idx:
            for key, val in opts.items():
                idx.set_option(key, val)
            idx.add(C)
            res.append(_check(idx, oracle, C, Q, k))
            _assert_unscreened(idx, B)
    _same(res[0], res[1])
    _same(res[0], res[2])


@pytest.mark.parametrize("order", ["ascending", "gauss"])
@pytest.mark.parametrize("growth", [1, 63])
@pytest.mark.parametrize("chunk0", [256, 4096, 100_000])
def test_chunk_ladder_options_on_the_unscreened_path(pkg, oracle, chunk0, growth, order):
    """chunk0_rows below, at twice and far above the 2048-slot list (the scan clamps its first chunk to the list) and
    growth 1 (doubling) or 63: chunks that fit, chunks that overflow and are re-run in pieces (ascending), and overflow
    checks that find nothing (gauss)"""
    C, Q = case(order, "zero")
    for k in (100, 1024):
        with pkg.Mi355Index(D) as idx:
            idx.set_option("chunk0_rows", chunk0)
            idx.set_option("chunk_growth", growth)
            idx.add(C)
            _check(idx, oracle, C, Q, k)
            _assert_unscreened(idx, B)


@pytest.mark.parametrize("screen", ["auto", "bf16"])
@pytest.mark.parametrize("n_irr,n_loose", [(1024, 0), (1025, 0), (1000, 40), (1024, 40)])
def test_irregular_row_limit(pkg, oracle, n_irr, n_loose, screen):
    """exactly kIrrCap irregular rows still screen, one more does not; loose rows count toward the int8 limit only
    (irregular + loose rows > 1024: the int8 screen is unavailable and AUTO screens with bf16).  k = 100, ascending."""
    k = 100
    C, Q = make_case("ascending", "mixed", n_irr=n_irr, n_loose=n_loose)
    with pkg.Mi355Index(D) as idx:
        idx.set_option("screen_dtype", screen)
        idx.add(C)
        assert idx.stat("irregular_rows") == n_irr
        assert idx.stat("loose_rows") >= n_irr + n_loose
        _check(idx, oracle, C, Q, k)
        active = idx.stat("screen_dtype_active")
        if screen == "bf16" or idx.stat("loose_rows") > 1024:
            assert active == 1
        else:
            assert active in (1, 2)
        if n_irr <= 1024:
            assert idx.stat("screen_launches") > 0
        else:
            assert idx.stat("screen_launches") == 0 and idx.stat("fallback_queries") == B


@pytest.mark.parametrize("row_offset", [0, 2**33])
def test_unscreened_blocks_in_flight(pkg, oracle, row_offset):
    """the async block API with several unscreened k = 100 blocks queued behind each other (the scan's overflow check
    synchronises on the host while later blocks wait to be enqueued), then waited for out of order"""
    k = 100
    C, Q = case("ascending", "mixed")
    blocks = [Q, Q[:1], Q[3:10], Q[::-1].copy(), Q[:2]]
    with pkg.Mi355Index(D) as idx:
        idx.add(C)
        idx.set_option("row_offset", row_offset)
        bufs = []
        for q in blocks:
            pq, od, orr = idx.dev_alloc(q.nbytes), idx.dev_alloc(len(q) * k * 8), idx.dev_alloc(len(q) * k * 8)
            idx.dev_upload(pq, q)
            bufs.append((pq, od, orr))
        tickets = [idx.search_device_async(pq, len(q), k, od, orr) for q, (pq, od, orr) in zip(blocks, bufs)]
        idx.search_wait(tickets[1])
        idx.search_wait(tickets[-1])
        for q, (pq, od, orr) in zip(blocks, bufs):
            gd, gr = np.empty((len(q), k)), np.empty((len(q), k), dtype=np.int64)
            idx.dev_download(od, gd)
            idx.dev_download(orr, gr)
            rd, rr = oracle.topk_search(C, q, k)
            _same((gd, gr), (rd, np.where(rr >= 0, rr + row_offset, rr)))
        _assert_unscreened(idx, sum(len(q) for q in blocks))
        for b in bufs:
            for p in b:
                idx.dev_free(p)
