"""GPU, two ranks on one MI355X over gloo (the pattern of tests/test_gpu_world2.py): `ShardedSearcher.maxsim_align` /
`maxsim_map` / `multivec_token_counts` over a store split by cumulative token count.  Every rank's result equals what one
index holding every document returns: value bits, token indices, distance bits, maps, counts."""

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
from autorag_research_amd.sharded import ShardedSearcher, shard_bounds_by_tokens
import maxsim_align_ref as ref

rank, world = int(os.environ["RANK"]), 2
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)

rng = np.random.default_rng(31)
d = 128
lens = rng.integers(0, 70, size=120)
lens[:10] = rng.integers(100, 160, size=10)      # a token-heavy head: the first shard is shorter in documents
tok = rng.standard_normal((int(lens.sum()), d)).astype(np.float32)
tok /= np.linalg.norm(tok, axis=1, keepdims=True)
off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
qlens = [32, 0, 5]
q = rng.standard_normal((sum(qlens), d)).astype(np.float32)
qo = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
ids = np.stack([rng.permutation(120)[:9] for _ in range(3)]).astype(np.int64)   # candidates from both shards, mixed
ids[0, 3], ids[2, 0], ids[2, 8] = -1, 120, ids[2, 1]
pq, pd = [0, 2, 2, 1, 0], [int(ids[0, 0]), 3, 119, 3, 500]

lo, hi = shard_bounds_by_tokens(off, world, rank)
assert 0 < hi - lo < 120
with pkg.Mi355Index(d) as whole:
    whole.add_multivec(tok, off)
    want = whole.maxsim_align(q, qo, ids), whole.maxsim_align(q, qo, ids, clamp0=True, want_dist=False), \
        whole.maxsim_map(q, qo, pq, pd), whole.multivec_token_counts(np.r_[ids.reshape(-1), 500])
s = ShardedSearcher(d, "cosine", device=0)
assert s.world == 2
s.add_local_multivec(tok[off[lo]:off[hi]], off[lo:hi + 1] - off[lo], lo)
ref.same_alignment(s.maxsim_align(q, qo, ids), want[0])
ref.same_alignment(s.maxsim_align(q, qo, ids, clamp0=True, want_dist=False), want[1])
got = s.maxsim_map(q, qo, pq, pd)
assert len(got) == len(want[2])
for a, b in zip(got, want[2]):
    ref.same_bits(a, b)
assert np.array_equal(s.multivec_token_counts(np.r_[ids.reshape(-1), 500]), want[3])
s.close()
dist.barrier()
dist.destroy_process_group()
print("ALIGN_WORLD2_OK", rank)
"""


def test_two_ranks_equal_one_store(native_built, oracle):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    script = _CHILD % {"root": str(ROOT), "tests": str(ROOT / "tests")}
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
    bad = [rank for rank, (p, (so, _)) in enumerate(zip(procs, outs)) if p.returncode != 0 or f"ALIGN_WORLD2_OK {rank}" not in so]
    if bad:   # (the rank that failed first is the one to read: its peer then dies in the next collective)
        pytest.fail("\n".join(f"rank {rank}: exit code {procs[rank].returncode}\n--- stdout\n{outs[rank][0][-800:]}\n--- stderr\n"
                              f"{outs[rank][1][-3500:]}" for rank in bad))
