"""GPU, one process: `mi355dr_search_collapsed_sharded_device` at world size 1 -- over the library's RCCL communicator (a child
process, as tests/test_gpu_shard_derived_world1.py) and over `mi355dr_comm_init_custom` with a copy-through transport
(in-process).  At one rank it must equal the local form bit for bit, with `row_offset` set (the key table is indexed by GLOBAL
rows), take the same re-searches, and refuse before the first collective."""

import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import collapse_ref as cr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
E_INVALID, E_UNSUPPORTED = -1, -4
OFFSET = 1000

_CASES = r"""
def make_index():
    C, Q, keys = cr.corpus_a()
    idx = pkg.Mi355Index(C.shape[1])
    idx.set_option("row_offset", OFFSET)
    idx.add(C)
    idx.remove_rows([1000, 17])                             # (local ids: a planted row and another)
    table = np.full(OFFSET + len(C), -1, dtype=np.int64)
    table[OFFSET:] = keys                                   # indexed by the global rows the searches return
    return idx, Q, table


def sharded_equals_local(idx, Q, table):
    for cap, k, fetch_k, max_fetch in ((1, 10, 16, 1024), (2, 10, 10, 1024), (3, 10, 1024, 1024), (1, 10, 16, 300), (1, 2, 2, 64)):
        idx.reset_stats()
        local = idx.search_collapsed(Q, k, cap, table, fetch_k, max_fetch)
        want = idx.stat("collapse_researched")
        idx.reset_stats()
        cr.same_search(idx.search_collapsed_sharded(Q, k, cap, table, fetch_k, max_fetch), local, f"cap={cap} f={fetch_k} m={max_fetch}")
        assert idx.stat("collapse_researched") == want and idx.stat("collapse_searches") == 1
    big = np.random.default_rng(9).standard_normal((1030, Q.shape[1])).astype(np.float32)   # two internal blocks
    big[[3, 1027]] = Q[0]
    cr.same_search(idx.search_collapsed_sharded(big, 10, 1, table, 16, 512), idx.search_collapsed(big, 10, 1, table, 16, 512), "B=1030")
    none = idx.search_collapsed_sharded(Q, 10, 1, None, 16, 1024)
    d, r = idx.search(Q, 10)
    assert np.array_equal(none.dist.view(np.uint64), d.view(np.uint64)) and np.array_equal(none.rows, r) and (r >= OFFSET).all()
"""

_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=%(port)r, RANK="0", WORLD_SIZE="1")
import torch
import torch.distributed as dist
import autorag_research_amd as pkg
from autorag_research_amd.sharded import ShardedSearcher
import collapse_ref as cr
OFFSET = 1000
"""

_CHILD_BODY = r"""
idx, Q, table = make_index()
idx.comm_init(0, 1, pkg.Mi355Index.comm_unique_id())
assert idx.comm_world() == 1
sharded_equals_local(idx, Q, table)

# ShardedSearcher over torch.distributed (nccl = RCCL): the library communicator is created lazily
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
C = cr.corpus_a()[0]
s = ShardedSearcher(C.shape[1], "cosine", device=0)
s.force_pipeline = True
s.add_local(C, OFFSET)
s.index.remove_rows([1000, 17])
assert s.index.comm_world() == 0
cr.same_search(s.search_collapsed(Q, 10, 1, table, 16, 1024), idx.search_collapsed(Q, 10, 1, table, 16, 1024), "ShardedSearcher")
assert s.index.comm_world() == 1 and s.index.stat("collapse_researched") == 5
s.close()
idx.close()
dist.destroy_process_group()
print("COLLAPSE1_OK")
"""


def test_rccl_communicator_at_world_one_equals_the_local_form(native_built):
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    script = _CHILD % {"root": str(ROOT), "tests": str(ROOT / "tests"), "port": port} + _CASES + _CHILD_BODY
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "COLLAPSE1_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.fixture(scope="module")
def cases(native_built):
    import autorag_research_amd as pkg

    ns = {"pkg": pkg, "np": np, "cr": cr, "OFFSET": OFFSET}
    exec(_CASES, ns)
    return ns


@pytest.fixture()
def looped(cases):
    """(index at row_offset 1000 over a copy-through transport at world 1, the transport's calls, Q, the key table)"""
    idx, Q, table = cases["make_index"]()
    calls = []

    def all_gather(send_ptr, recv_ptr, nbytes, stream):
        tmp = np.empty(nbytes // 8, dtype=np.int64)
        idx.dev_download(send_ptr, tmp)
        idx.dev_upload(recv_ptr, tmp)
        calls.append(nbytes)

    idx.comm_init_custom(0, 1, all_gather)
    yield idx, calls, Q, table
    idx.close()


def test_custom_transport_at_world_one_equals_the_local_form(cases, looped):
    idx, calls, Q, table = looped
    cases["sharded_equals_local"](idx, Q, table)
    assert calls and all(b % 8 == 0 for b in calls)
    # one gather per round: the block at 16, then the one unfinished query at 32 .. 512
    del calls[:]
    idx.search_collapsed_sharded(Q, 10, 1, table, 16, 1024)
    assert calls == [8 * 2 * 5 * 16] + [8 * 2 * 1 * f for f in (32, 64, 128, 256, 512)]


def test_refusals_come_before_the_first_collective(cases, looped):
    import autorag_research_amd as pkg

    idx, calls, Q, table = looped

    def refused(fn, code, text):
        with pytest.raises(pkg.NativeError, match=text) as e:
            fn()
        assert e.value.code == code

    with pkg.Mi355Index(Q.shape[1]) as bare:
        bare.add(np.zeros((10, Q.shape[1]), np.float32) + 1)
        refused(lambda: bare.search_collapsed_sharded(Q, 5, 1, table, 8, 64), E_INVALID, "mi355dr_comm_init has not been called")
    view = idx.view(row_ids=np.arange(OFFSET, OFFSET + 200))
    try:
        refused(lambda: view.search_collapsed_sharded(Q, 5, 1, table, 8, 64), E_INVALID, "ask the parent")
        cr.same_search(view.search_collapsed(Q, 5, 1, table, 8, 64),                       # (the local form serves a view)
                       cr.search_result(*view.search(Q, 64), table, 1, 5, 64), "local on a view")
    finally:
        view.close()
    refused(lambda: idx.search_collapsed_sharded(Q, 5, 1, table, 8, 1025), E_UNSUPPORTED, "exceeds 1024")
    refused(lambda: idx.search_collapsed_sharded(Q, 5, 0, table, 8, 64), E_INVALID, "cap")
    refused(lambda: idx.search_collapsed_sharded(Q, 5, 1, table, 4, 64), E_INVALID, "fetch_k")
    refused(lambda: idx.search_collapsed_sharded(Q, 5, 1, table, 80, 64), E_INVALID, "max_fetch")
    assert calls == []
    got = idx.search_collapsed_sharded(np.zeros((0, Q.shape[1]), np.float32), 5, 1, table, 8, 64)   # B == 0: no collective
    assert got.rows.shape == (0, 5) and calls == []
