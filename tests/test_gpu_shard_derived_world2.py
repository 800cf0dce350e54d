"""GPU, TWO ranks on ONE MI355X over gloo (the form of tests/test_gpu_world2.py): the range, by-row and MMR searches of a
row-sharded index, inside the library (`mi355dr_search_*_sharded_device`, `mi355dr_mmr_select_sharded`) over
`mi355dr_comm_init_custom` with a gloo all-gather as the transport, and through `ShardedSearcher`.  Every rank's result == what
ONE index holding all rows returns == the CPU references of tests/range_ref.py, rows_ref.py and mmr_ref.py: rows and NaN masks
equal, float8 bits equal, counts equal.  One pair of processes per test function, every case inside the child."""

import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

_PRELUDE = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import torch
import torch.distributed as dist
import autorag_research_amd as pkg
from autorag_research_amd.sharded import ShardedSearcher, shard_bounds
from oracle import cpu_ref
import range_ref, rows_ref, mmr_ref

rank, world = int(os.environ["RANK"]), 2
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)
INF = float("inf")


class Shard:
    # this rank's rows [lo, hi) of C twice: a Mi355Index over a RECORDING gloo transport (the C-level methods) and a
    # ShardedSearcher (its own lazily created library communicator); the rows in `removed` (global) removed after the add
    def __init__(self, C, lo, hi, metric, removed):
        d = C.shape[1]
        mine = np.array([r - lo for r in removed if lo <= r < hi], dtype=np.int64)
        self.idx = pkg.Mi355Index(d, metric)
        self.idx.set_option("row_offset", lo)
        self.s = ShardedSearcher(d, metric, device=0)
        self.s.row_offset = lo
        self.s.index.set_option("row_offset", lo)
        for ix in (self.idx, self.s.index):
            if hi > lo:
                ix.add(C[lo:hi])
            if mine.size:
                ix.remove_rows(mine)
        self.calls = []

        def all_gather(send_ptr, recv_ptr, nbytes, stream):
            assert nbytes %% 8 == 0
            part = np.empty(nbytes // 8, dtype=np.int64)
            self.idx.dev_download(send_ptr, part)
            out = torch.empty(world * part.size, dtype=torch.int64)
            dist.all_gather_into_tensor(out, torch.from_numpy(part))
            self.idx.dev_upload(recv_ptr, out.numpy())
            self.calls.append(nbytes)

        self.idx.comm_init_custom(rank, world, all_gather)

    def both(self, c_level, searcher):
        # the same case through the C-level method of the index and through ShardedSearcher
        return [("C ABI", c_level(self.idx)), ("ShardedSearcher", searcher(self.s))]

    def close(self):
        self.idx.close()
        self.s.close()


def rows_payload(nb, d):      # include/mi355dr.h: nb x d floats, nb int32 valid, nb double self distances, each padded to 8 bytes
    return 8 * ((nb * d + 1) // 2 + (nb + 1) // 2 + nb)


def stage_bytes(nq, width, d):  # one rank's MMR stage of a sub-block: round_up4(nq x width x (d + 2)) floats
    return 4 * ((nq * width * (d + 2) + 3) // 4 * 4)


def whole_index(C, metric, removed):
    w = pkg.Mi355Index(C.shape[1], metric)
    w.add(C)
    if len(removed):
        w.remove_rows(np.asarray(removed, dtype=np.int64))
    return w


def range_and_rows_cases(C, Q, metric, removed, ids, sh, lo1, m_list, k_list):
    # the range and by-row cases of one corpus; returns nothing, asserts everything
    n = len(C)
    live = np.ones(n, dtype=bool)
    live[removed] = False
    ds, rs = range_ref.oracle_sorted(cpu_ref, C, Q, metric)
    B = len(Q)
    crossed = False
    for m in m_list:
        want = np.array([0, 3, m + 5, 3, m + 5, 3, 3][:B])
        radius, counts = range_ref.radius_admitting(ds, rs, want, live)
        assert (counts == 0).any() and (counts == 3).any() and (counts > m).any()   # (one count exceeds the list)
        for r in (radius, np.where(np.arange(B) == 1, INF, np.where(np.arange(B) == 3, -INF, radius))):
            exp = range_ref.search_range(ds, rs, r, m, live)
            in_range = [exp[1][b][exp[1][b] >= 0] for b in range(B)]
            crossed |= any((x < lo1).any() and (x >= lo1).any() for x in in_range)
            for name, got in sh.both(lambda ix: ix.search_range_sharded(Q, r, m), lambda s: s.search_range(Q, r, m)):
                range_ref.same(got, exp)
    assert crossed, "vacuous: no query's in-range rows came from both shards"

    # ---- by stored row
    valid = rows_ref._slots(C, ids, live, 0)[1]
    n_bad = int((~valid).sum())
    assert n_bad == 3                                                # the removed row, the id beyond the corpus, -1
    for k in k_list:
        for inc in (False, True):
            exp = rows_ref.search_rows(cpu_ref, C, ids, k, metric, live, inc)
            for ix in (sh.idx, sh.s.index):
                ix.reset_stats()
            for name, got in sh.both(lambda ix: ix.search_rows_sharded(ids, k, inc), lambda s: s.search_rows(ids, k, inc)):
                rows_ref.same(got, exp)
            assert sh.idx.stat("rows_skipped") == n_bad and sh.s.index.stat("rows_skipped") == n_bad   # (on BOTH ranks)
            assert sh.idx.stat("sharded_rows_searches") == 1 and sh.idx.stat("rows_queries") == len(ids)
    # the range form: radii that admit about 3 and max_results + 5 rows of each valid slot, +inf, -inf, and nothing at all
    local = np.where(valid, ids, 0)
    near = cpu_ref.topk_search(C, np.ascontiguousarray(C[local]), 40, metric=metric)[0]
    for m in m_list:
        for inc in (False, True):
            radius = np.where(np.arange(len(ids)) %% 2 == 0, near[:, 4], near[:, m + 6])
            radius = np.where(np.isnan(radius), 0.5, radius)         # (the zero row under cosine has no distances)
            radius[1], radius[3] = INF, -INF
            exp = rows_ref.search_range_rows(cpu_ref, C, ids, radius, m, metric, live, inc)
            assert (exp[2] > m).any() and (exp[2] == 0).any()
            sh.idx.reset_stats()
            for name, got in sh.both(lambda ix: ix.search_range_rows_sharded(ids, radius, m, inc),
                                     lambda s: s.search_range_rows(ids, radius, m, inc)):
                rows_ref.same(got, exp)
            assert sh.idx.stat("rows_skipped") == n_bad
"""

_CHILD_COSINE = _PRELUDE + r"""
rng = np.random.default_rng(2024)
n, d, B = 20_000, 100, 7                      # d is no multiple of 4: the scalar copy paths and mmr_dq's rounding
C = rng.standard_normal((n, d)).astype(np.float32)
lo, hi = shard_bounds(n, world, rank, granule=256)
lo1 = shard_bounds(n, world, 1, granule=256)[0]
A, TWIN, LOWER, ZERO = 123, lo1 + 77, 40, 500
C[TWIN] = C[A]                                # an exact copy of a shard-0 row on shard 1 ...
C[LOWER] = C[A]                               # ... and one at a lower id on the same shard
C[ZERO] = 0.0
removed = [900, lo1 + 900]                    # one row removed on each shard after the add
Q = rng.standard_normal((B, d)).astype(np.float32)
Q[2] = C[A] + 0.01 * rng.standard_normal(d).astype(np.float32)   # looks at the copies on both shards
sh = Shard(C, lo, hi, "cosine", removed)
ids = np.array([A, lo1 + 5, TWIN, LOWER, ZERO, removed[0], n + 5, -1, lo1 + 5], dtype=np.int64)
range_and_rows_cases(C, Q, "cosine", removed, ids, sh, lo1, (1, 10), (1, 10))
# self excluded, the twin present at distance 0 (asserted on the reference: the case cannot go vacuous)
exp = rows_ref.search_rows(cpu_ref, C, ids, 10, "cosine", np.isin(np.arange(n), removed, invert=True), False)
assert LOWER in exp[1][0][:2] and TWIN in exp[1][0][:2] and A not in exp[1][0] and A in exp[1][2][:2] and TWIN not in exp[1][2]

# B = 1100: two internal blocks (against the unsharded index over the whole corpus)
big = rng.integers(-3, n + 3, size=1100)
with whole_index(C, "cosine", removed) as whole:
    exp = whole.search_rows(big, 3)
    rows_ref.same(sh.idx.search_rows_sharded(big, 3), exp)

# gather bytes: the transport saw exactly the documented payloads, and the stat counts what this rank received
sh.idx.reset_stats()
del sh.calls[:]
radius = np.full(B, 0.9)
sh.idx.search_range_sharded(Q, radius, 10)
sh.idx.search_rows_sharded(ids, 10)
sh.idx.search_range_rows_sharded(ids, np.full(len(ids), 0.9), 10)
sh.idx.search_rows_sharded(big, 3, True)
expect = [8 * (2 * B * 10 + B),
          rows_payload(9, d), 8 * 2 * 9 * 11,
          rows_payload(9, d), 8 * (2 * 9 * 11 + 9),
          rows_payload(1024, d), 8 * 2 * 1024 * 3, rows_payload(76, d), 8 * 2 * 76 * 3]
assert sh.calls == expect, (sh.calls, expect)
assert sh.idx.stat("shard_gather_bytes") == world * sum(expect)
assert sh.idx.stat("sharded_range_searches") == 1 and sh.idx.stat("sharded_rows_searches") == 3
sh.close()
dist.barrier()
dist.destroy_process_group()
print("SHARD2_OK", rank)
"""

_CHILD_IP = _PRELUDE + r"""
rng = np.random.default_rng(31)
n, d, B = 6_000, 256, 7                       # the core cases once more: d = 256 (the float4 copies), inner product
C = rng.standard_normal((n, d)).astype(np.float32)
lo, hi = shard_bounds(n, world, rank, granule=256)
lo1 = shard_bounds(n, world, 1, granule=256)[0]
A, TWIN, LOWER, ZERO = 123, lo1 + 77, 40, 500
C[TWIN] = C[A]
C[LOWER] = C[A]
C[ZERO] = 0.0
removed = [900, lo1 + 900]
Q = rng.standard_normal((B, d)).astype(np.float32)
sh = Shard(C, lo, hi, "ip", removed)
ids = np.array([A, lo1 + 5, TWIN, LOWER, ZERO, removed[0], n + 5, -1, lo1 + 5], dtype=np.int64)
range_and_rows_cases(C, Q, "ip", removed, ids, sh, lo1, (10,), (10,))
# MMR under inner product
live = np.isin(np.arange(n), removed, invert=True)
k, fetch_k = 5, 40
dd, rr = cpu_ref.topk_search(C, Q, fetch_k + len(removed), metric="ip")
keep = [np.flatnonzero(live[rr[b]])[:fetch_k] for b in range(B)]
cd = np.stack([dd[b][keep[b]] for b in range(B)])
cr = np.stack([rr[b][keep[b]] for b in range(B)])
for lam in (0.0, 0.5, 1.0):
    exp = mmr_ref.mmr_from_lists(cpu_ref, C, cd, cr, k, lam, "ip")
    for name, got in sh.both(lambda ix: ix.search_mmr_sharded(Q, k, fetch_k, lam), lambda s: s.search_mmr(Q, k, fetch_k, lam)):
        mmr_ref.same(got, exp)
sh.close()
dist.barrier()
dist.destroy_process_group()
print("SHARD2_OK", rank)
"""

_CHILD_MMR = _PRELUDE + r"""
d, B, k, fetch_k = 100, 7, 5, 40
C, Q = mmr_ref.clustered(d, B)                # near-copies in clusters: the picks leave the top-k
n = len(C)
lo, hi = shard_bounds(n, world, rank, granule=256)
lo1 = shard_bounds(n, world, 1, granule=256)[0]
d0, r0 = cpu_ref.topk_search(C, Q, fetch_k + 2)
removed = [int(r0[0][r0[0] < lo1][1]), int(r0[1][r0[1] >= lo1][1])]   # one candidate of a query on each shard
live = np.isin(np.arange(n), removed, invert=True)
keep = [np.flatnonzero(live[r0[b]])[:fetch_k] for b in range(B)]
cd = np.stack([d0[b][keep[b]] for b in range(B)])
cr = np.stack([r0[b][keep[b]] for b in range(B)])
assert all(((cr[b] < lo1).any() and (cr[b] >= lo1).any()) for b in range(B))   # every list draws on both shards
sh = Shard(C, lo, hi, "cosine", removed)
# the gathered stage holds three queries: B = 7 runs in sub-blocks of 3, 3 and 1
cap = world * stage_bytes(3, fetch_k, d) + 16
for ix in (sh.idx, sh.s.index):
    ix.set_option("shard_stage_bytes", cap)
for lam in (0.0, 0.5, 1.0):
    exp = mmr_ref.mmr_from_lists(cpu_ref, C, cd, cr, k, lam)
    if lam == 0.5:
        assert not np.array_equal(exp[1], cr[:, :k]), "vacuous: MMR picked the plain top-k"
    if lam == 1.0:
        assert np.array_equal(exp[1], cr[:, :k])                   # the sharded top-k over the eligible candidates
    sh.idx.reset_stats()
    del sh.calls[:]
    for name, got in sh.both(lambda ix: ix.search_mmr_sharded(Q, k, fetch_k, lam), lambda s: s.search_mmr(Q, k, fetch_k, lam)):
        mmr_ref.same(got, exp)
    expect = [8 * 2 * B * fetch_k, stage_bytes(3, fetch_k, d), stage_bytes(3, fetch_k, d), stage_bytes(1, fetch_k, d)]
    assert sh.calls == expect, (sh.calls, expect)
    assert sh.idx.stat("shard_gather_bytes") == world * sum(expect) and sh.idx.stat("sharded_mmr_searches") == 1
    assert sh.idx.stat("mmr_queries") == B and sh.idx.stat("mmr_pairs_scored") == exp[2]

# the caller's pools: rows of both shards, a removed row, -1 padding and a duplicate
pools = np.stack([np.concatenate([cr[b][:9], [removed[b %% 2], -1, cr[b][0]]]) for b in range(B)]).astype(np.int64)
assert all(((p[:9] < lo1).any() and (p[:9] >= lo1).any()) for p in pools)
m = pools.shape[1]
for kk, lam in ((5, 0.5), (5, 0.0), (20, 0.5)):                    # k = 20: more than the eligible candidates
    exp = mmr_ref.mmr_select(cpu_ref, C, Q, kk, pools, lam, live=live)
    assert kk != 20 or (exp[1][:, 9:] == -1).all()
    del sh.calls[:]
    for name, got in sh.both(lambda ix: ix.mmr_select_sharded(Q, kk, pools, lam), lambda s: s.mmr_select(Q, kk, pools, lam)):
        mmr_ref.same(got, exp)
    assert sh.calls == [8 * 2 * B * m, stage_bytes(B, m, d)], sh.calls   # (all seven pools fit the stage at this width)
sh.close()
dist.barrier()
dist.destroy_process_group()
print("SHARD2_OK", rank)
"""

_CHILD_EMPTY = _PRELUDE + r"""
rng = np.random.default_rng(5)
n, d, B = 300, 100, 4                         # a tiny corpus of which rank 1 holds no row
C = rng.standard_normal((n, d)).astype(np.float32)
Q = rng.standard_normal((B, d)).astype(np.float32)
lo, hi = (0, n) if rank == 0 else (n, n)
sh = Shard(C, lo, hi, "cosine", [])
assert len(sh.idx) == (n if rank == 0 else 0)
ids = np.array([5, 299, 300, -1], dtype=np.int64)
pools = rng.integers(0, n, size=(B, 12))
with whole_index(C, "cosine", []) as whole:
    radius = whole.search(Q, 6)[0][:, 5]
    for name, got in sh.both(lambda ix: ix.search_range_sharded(Q, radius, 4), lambda s: s.search_range(Q, radius, 4)):
        range_ref.same(got, whole.search_range(Q, radius, 4))
    for name, got in sh.both(lambda ix: ix.search_rows_sharded(ids, 3), lambda s: s.search_rows(ids, 3)):
        rows_ref.same(got, whole.search_rows(ids, 3))
    r4 = np.full(4, 0.95)
    for name, got in sh.both(lambda ix: ix.search_range_rows_sharded(ids, r4, 3), lambda s: s.search_range_rows(ids, r4, 3)):
        rows_ref.same(got, whole.search_range_rows(ids, r4, 3))
    for name, got in sh.both(lambda ix: ix.search_mmr_sharded(Q, 3, 10, 0.5), lambda s: s.search_mmr(Q, 3, 10, 0.5)):
        mmr_ref.same(got, whole.search_mmr(Q, 3, 10, 0.5))
    for name, got in sh.both(lambda ix: ix.mmr_select_sharded(Q, 3, pools, 0.5), lambda s: s.mmr_select(Q, 3, pools, 0.5)):
        mmr_ref.same(got, whole.mmr_select(Q, 3, pools, 0.5))
    assert sh.idx.stat("rows_skipped") == 4                        # ids 300 and -1, in both by-row calls, on both ranks
sh.close()
dist.barrier()
dist.destroy_process_group()
print("SHARD2_OK", rank)
"""


def _run_pair(child):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    script = child % {"root": str(ROOT), "tests": str(ROOT / "tests")}
    procs = []
    for rank in range(2):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank),
                   WORLD_SIZE="2", OMP_NUM_THREADS="8")
        procs.append(subprocess.Popen([sys.executable, "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=600))
        except subprocess.TimeoutExpired:
            for pp in procs:
                pp.kill()
            raise
    bad = [rank for rank, (p, (so, _)) in enumerate(zip(procs, outs)) if p.returncode != 0 or f"SHARD2_OK {rank}" not in so]
    # (the rank that failed FIRST is the one to read: its peer then dies in the next collective)
    return "\n".join(f"rank {rank}: exit code {procs[rank].returncode}\n--- stdout\n{outs[rank][0][-800:]}\n--- stderr\n"
                     f"{outs[rank][1][-3500:]}" for rank in bad)


def _check(child):
    report = _run_pair(child)
    if report and "AssertionError" not in report and "NativeError" not in report:
        # a rank lost to the rendezvous is not a verdict on the search: one more attempt; a parity failure (an assert, a library
        # error) never retries
        report = _run_pair(child)
    if report:
        pytest.fail(report)


def test_range_and_by_row_search_on_two_shards(native_built, oracle):
    _check(_CHILD_COSINE)


def test_mmr_search_and_select_on_two_shards(native_built, oracle):
    _check(_CHILD_MMR)


def test_core_cases_at_d256_inner_product(native_built, oracle):
    _check(_CHILD_IP)


def test_a_rank_without_rows_still_enters_every_collective(native_built, oracle):
    _check(_CHILD_EMPTY)
