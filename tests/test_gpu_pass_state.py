"""A search pass takes what it decided as a value: passes nested in one another and fix-ups that run behind blocks of another
k leave every block the oracle's answer, bit for bit, and leave the caller's options alone."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, B = 6000, 64, 20


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(46)
    C = rng.standard_normal((N, D)).astype(np.float32)
    Q = rng.standard_normal((B, D)).astype(np.float32)
    return C, Q


def _same(dist, rows, rd, rr):
    assert np.array_equal(rows, rr)
    assert np.array_equal(np.isnan(dist), np.isnan(rd))  # NaN payload/sign is not part of the contract
    ok = ~np.isnan(rd)
    assert np.array_equal(dist[ok].view(np.uint64), rd[ok].view(np.uint64))


class _AsyncBlocks:
    """blocks enqueued back to back with search_device_async; check() after the wait compares each with the oracle"""

    def __init__(self, idx):
        self.idx, self.blocks, self.tickets = idx, [], []

    def enqueue(self, Q, k):
        idx = self.idx
        pq, od, orr = idx.dev_alloc(Q.nbytes), idx.dev_alloc(len(Q) * k * 8), idx.dev_alloc(len(Q) * k * 8)
        idx.dev_upload(pq, Q)
        self.blocks.append((Q, k, pq, od, orr))
        self.tickets.append(idx.search_device_async(pq, len(Q), k, od, orr))

    def check(self, oracle, C):
        for Q, k, pq, od, orr in self.blocks:
            gd, gr = np.empty((len(Q), k)), np.empty((len(Q), k), dtype=np.int64)
            self.idx.dev_download(od, gd)
            self.idx.dev_download(orr, gr)
            _same(gd, gr, *oracle.topk_search(C, Q, k))
            for p in (pq, od, orr):
                self.idx.dev_free(p)


def test_fixups_behind_blocks_of_another_k(pkg, oracle, data):
    """Four asynchronous blocks at k = 10, 100, 200, 10 (the one-wave, the two-wave and the general prune), each with one
    all-zero query: the screen cannot rank it, so each block's exact scan runs at the wait, after the blocks of the other k
    were enqueued behind it."""
    C, Q = data
    with pkg.Mi355Index(D) as fresh:
        fresh.add(C)
        fresh.search(Q, 10)
        dtype_at_10 = fresh.stat("screen_dtype_active")
    with pkg.Mi355Index(D) as idx:
        idx.add(C)
        idx.reset_stats()
        run = _AsyncBlocks(idx)
        for j, k in enumerate((10, 100, 200, 10)):
            Qj = np.roll(Q, j, axis=0).copy()
            Qj[3 + j] = 0.0
            run.enqueue(Qj, k)
        idx.search_wait(run.tickets[-1])
        run.check(oracle, C)
        assert idx.stat("fallback_queries") == 4
        assert idx.stat("screen_dtype_active") == dtype_at_10


def _overflow_fixups(idx, oracle, C, Q):
    """16-slot candidate lists at k = 10: two asynchronous blocks, a blocking range search behind them, then the wait"""
    idx.set_option("cand_cap", 16)
    idx.reset_stats()
    run = _AsyncBlocks(idx)
    run.enqueue(Q, 10)
    run.enqueue(Q[::-1].copy(), 10)
    rdist, rrows, rcount = idx.search_range(Q, np.inf, 5)
    idx.search_wait(run.tickets[-1])
    run.check(oracle, C)
    _same(rdist, rrows, *idx.search(Q, 5))
    assert (rcount == N).all()
    assert idx.stat("retry_queries") > 0 and idx.stat("fallback_queries") > 0


def test_overflow_fixups_around_a_range_pass(pkg, oracle, data):
    """Every list overflows: the blocks' re-screens and exact scans run inside the range search's call, and the range pass
    itself hands its queries (all 6000 rows are in range) to an ordinary pass with fix-ups of its own."""
    C, Q = data
    with pkg.Mi355Index(D) as idx:
        idx.add(C)
        _overflow_fixups(idx, oracle, C, Q)


def test_option_path_is_the_callers(pkg, oracle, data):
    """The fix-ups run exact scans of their own; option "path" stays what the caller set.  path = screen is still refused on a
    corpus no screen can serve, and path = auto still screens an ordinary one."""
    C, Q = data
    with pkg.Mi355Index(D) as idx:
        idx.set_option("path", "screen")
        idx.add(C)
        _overflow_fixups(idx, oracle, C, Q)
        idx.add(np.zeros((1100, D), dtype=np.float32))  # more irregular rows than the screens tolerate (1024)
        with pytest.raises(pkg.NativeError, match="screen path unavailable"):
            idx.search(Q, 10)
    with pkg.Mi355Index(D) as idx:
        idx.add(C)
        _overflow_fixups(idx, oracle, C, Q)
        idx.set_option("path", "auto")
        idx.set_option("cand_cap", 2048)
        idx.reset_stats()
        _same(*idx.search(Q, 10), *oracle.topk_search(C, Q, 10))
        assert idx.stat("fallback_queries") == 0
