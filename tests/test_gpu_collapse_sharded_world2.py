"""GPU, TWO ranks on ONE MI355X over gloo (the form of tests/test_gpu_sparse_sharded_world2.py, its retry rule included): the source-capped search of a
row-sharded index -- `mi355dr_search_collapsed_sharded_device` over `mi355dr_comm_init_custom` with a gloo all-gather as the
transport, and through `ShardedSearcher` -- on two UNEVEN shards of corpus A against ONE index holding every row: results,
states and `collapse_researched` equal on both ranks.  One pair of processes, every case inside the child."""

import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import torch
import torch.distributed as dist
import autorag_research_amd as pkg
from autorag_research_amd.sharded import ShardedSearcher
import collapse_ref as cr

rank, world = int(os.environ["RANK"]), 2
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)

C, Q, keys = cr.corpus_a()
n, d = C.shape
CUT = 1100                                     # uneven shards; the heavy source (rows 1000 .. 1299) lies on BOTH
lo, hi = (0, CUT) if rank == 0 else (CUT, n)
removed = [1004, 1200, 3000]                   # global rows, removed on their owners after the add

idx = pkg.Mi355Index(d)
idx.set_option("row_offset", lo)
s = ShardedSearcher(d, "cosine", device=0)
s.row_offset = lo
s.index.set_option("row_offset", lo)
mine = np.array([r - lo for r in removed if lo <= r < hi], dtype=np.int64)
for ix in (idx, s.index):
    ix.add(C[lo:hi])
    ix.remove_rows(mine)
calls = []


def all_gather(send_ptr, recv_ptr, nbytes, stream):
    assert nbytes %% 8 == 0
    part = np.empty(nbytes // 8, dtype=np.int64)
    idx.dev_download(send_ptr, part)
    out = torch.empty(world * part.size, dtype=torch.int64)
    dist.all_gather_into_tensor(out, torch.from_numpy(part))
    idx.dev_upload(recv_ptr, out.numpy())
    calls.append(nbytes)


idx.comm_init_custom(rank, world, all_gather)
whole = pkg.Mi355Index(d)
whole.add(C)
whole.remove_rows(np.asarray(removed, dtype=np.int64))
full = whole.search(Q, 1024)
assert ((full[1][0][:300] < CUT).any() and (full[1][0][:300] >= CUT).any())      # query 0's list draws on both shards

for cap, k, fetch_k, max_fetch in ((1, 10, 16, 1024), (2, 10, 10, 1024), (3, 10, 300, 1024), (1, 10, 1024, 1024),
                                   (1, 10, 16, 300), (1, 2, 2, 2048 // world)):
    whole.reset_stats()
    exp = whole.search_collapsed(Q, k, cap, keys, fetch_k, max_fetch)
    want = whole.stat("collapse_researched")
    cr.same_search(exp, cr.search_result(full[0], full[1], keys, cap, k, max_fetch), "the whole index against the walk")
    assert want == cr.expected_researched(full[1], keys, cap, k, fetch_k, max_fetch)
    for name, ix, call in (("C ABI", idx, lambda: idx.search_collapsed_sharded(Q, k, cap, keys, fetch_k, max_fetch)),
                           ("ShardedSearcher", s.index, lambda: s.search_collapsed(Q, k, cap, keys, fetch_k, max_fetch))):
        ix.reset_stats()
        cr.same_search(call(), exp, f"{name} cap={cap} k={k} f={fetch_k} m={max_fetch}")
        assert ix.stat("collapse_researched") == want, (name, cap, fetch_k, max_fetch)
        assert ix.stat("collapse_truncated") == whole.stat("collapse_truncated")
assert whole.stat("collapse_truncated") == 0

# the gathers of one call: the block at 16, then the ONE unfinished query at 32 .. 512, each rank's [2, n, f] block
del calls[:]
idx.search_collapsed_sharded(Q, 10, 1, keys, 16, 1024)
assert calls == [8 * 2 * 5 * 16] + [8 * 2 * 1 * f for f in (32, 64, 128, 256, 512)], calls

# a table on the device, uploaded once; 1030 queries: two internal blocks
big = np.random.default_rng(3).standard_normal((1030, d)).astype(np.float32)
big[[1, 1025]] = Q[0]
with idx.upload_keys(keys) as table:
    cr.same_search(idx.search_collapsed_sharded(big, 10, 1, table, 16, 512), whole.search_collapsed(big, 10, 1, keys, 16, 512), "B=1030")

# a refusal comes on both ranks before any collective (world x max_fetch <= 4096 cannot fail at two ranks: max_fetch <= 1024)
del calls[:]
for bad, code in (((Q, 10, 1, keys, 16, 1025), -4), ((Q, 10, 1, keys, 9, 1024), -1), ((Q, 10, 0, keys, 16, 1024), -1)):
    try:
        idx.search_collapsed_sharded(*bad)
        raise SystemExit("not refused")
    except pkg.NativeError as e:
        assert e.code == code, e
assert calls == []
idx.close()
s.close()
whole.close()
dist.barrier()
dist.destroy_process_group()
print("COLLAPSE2_OK", rank)
"""


# what a lost rendezvous looks like in a child's stderr: the only failure that earns a second attempt
_RENDEZVOUS = ("DistNetworkError", "DistStoreError", "Connection refused", "Address already in use", "EADDRINUSE",
               "Connection reset by peer", "failed to connect")
# ... and what never does, whatever else the report holds: a verdict on the search, a library error, a GPU fault
_NEVER = ("AssertionError", "NativeError", "illegal memory access", "HSA_STATUS_ERROR", "Memory access fault")


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
            outs.append(p.communicate(timeout=300))
        except subprocess.TimeoutExpired:
            for pp in procs:
                pp.kill()
            raise
    bad = [rank for rank, (p, (so, _)) in enumerate(zip(procs, outs)) if p.returncode != 0 or f"COLLAPSE2_OK {rank}" not in so]
    # (the rank that failed FIRST is the one to read: its peer then dies in the next collective)
    report = "\n".join(f"rank {rank}: exit code {procs[rank].returncode}\n--- stdout\n{outs[rank][0][-800:]}\n--- stderr\n"
                       f"{outs[rank][1][-3500:]}" for rank in bad)
    # a rank that died of a signal (a fault, an abort: a negative exit code) is never a lost rendezvous
    lost = bool(bad) and all(procs[rank].returncode > 0 for rank in bad) and any(t in report for t in _RENDEZVOUS) \
        and not any(t in report for t in _NEVER)
    return report, lost


def test_search_collapsed_on_two_uneven_shards(native_built):
    report, lost = _run_pair(_CHILD)
    if report and lost:
        report, _ = _run_pair(_CHILD)      # one more attempt, for a lost rendezvous only
    if report:
        pytest.fail(report)
