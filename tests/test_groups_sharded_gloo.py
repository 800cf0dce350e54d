"""CPU, world_size 2 over gloo: ShardedSearcher.search_groups -- the sharded search at fetch_k, then the grouped merge on every
rank without a further collective -- equals the grouped merge of the unsharded oracle's lists (tests/groups_ref.py)."""

import os
import socket
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
OFFSETS = [0, 3, 3, 4, 9]   # ragged groups, one of them empty
K, FETCH_K = 14, 8


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _case():
    rng = np.random.default_rng(456)
    n, d = 2001, 48
    C = rng.standard_normal((n, d)).astype(np.float32)
    C[5] = C[1900]        # a cross-shard exact tie
    C[17] = 0.0           # a NaN distance with a row
    base = C[rng.integers(0, n, 3).repeat(3)]
    Q = (base + 0.3 * rng.standard_normal(base.shape)).astype(np.float32)
    return C, Q


def _worker(rank: int, world: int, port: int, out_dir: str):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    from helpers import OracleIndex
    from autorag_research_amd.sharded import ShardedSearcher, shard_bounds

    dist.init_process_group("gloo", rank=rank, world_size=world)
    C, Q = _case()
    lo, hi = shard_bounds(C.shape[0], world, rank, granule=250)
    s = ShardedSearcher(C.shape[1], "cosine", index_factory=OracleIndex)
    s.add_local(C[lo:hi], lo)
    assert not hasattr(s.index, "merge_groups")   # the stand-in has no device merge: merge_groups_host serves it
    dv, dr, dc = s.search_groups(Q, OFFSETS, K, FETCH_K)
    d1, r1, c1 = s.search_groups(Q, OFFSETS, 3)   # fetch_k defaults to k
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), d=dv, r=dr, c=dc, d1=d1, r1=r1, c1=c1)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_search_groups_equals_unsharded(tmp_path, oracle):
    import torch.multiprocessing as mp

    import groups_ref

    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    C, Q = _case()
    want = groups_ref.merge_groups(*oracle.topk_search(C, Q, FETCH_K), OFFSETS, K)
    want1 = groups_ref.merge_groups(*oracle.topk_search(C, Q, 3), OFFSETS, 3)
    assert want[2].tolist()[1] == 0 and want[2].max() > FETCH_K
    for rank in range(world):
        o = np.load(tmp_path / f"r{rank}.npz")
        groups_ref.same((o["d"], o["r"], o["c"]), want)
        groups_ref.same((o["d1"], o["r1"], o["c1"]), want1)
