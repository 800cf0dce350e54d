"""CPU: MaxSim search within a listed subset of documents -- the host layers over an oracle-backed index.

`ShardedSearcher.search_maxsim_subset` under gloo at world 2 (every rank passes the same global list and keeps what falls in
its shard; one all-gather of the packed [2, B, k] block, host merge) and the service's `within=` in `search_mode="multi"`,
which takes ONE `search_maxsim_subset` call where the searcher has the method and the `maxsim_subset` + host ordering recipe
where it has not.  The index stand-in answers by the oracle recipe of the restricted search: the listed documents with vectors,
unique and ascending, `maxsim_topk` over only those, rows mapped back through the ids -- positions are in id order, so the tie
rule (distance, then document) carries over."""

import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import OracleIndex

ROOT = Path(__file__).resolve().parent.parent


class OracleMaxsimSubsetIndex(OracleIndex):
    """OracleIndex + Mi355Index.search_maxsim_subset (global ids; ids outside the index and documents without vectors skipped)"""

    calls = None   # a dict the service tests hang here to count calls

    def search_maxsim_subset(self, qtok, q_offsets, k, doc_ids):
        if self.calls is not None:
            self.calls["search_maxsim_subset"] += 1
        q_offsets = np.asarray(q_offsets, dtype=np.int32)
        B = q_offsets.shape[0] - 1
        dist, rows = np.full((B, k), np.nan, np.float32), np.full((B, k), -1, np.int64)
        off = self._off if self._off is not None else np.zeros(1, np.int64)
        ids = np.unique(np.asarray(doc_ids, dtype=np.int64).reshape(-1) - self.row_offset)
        ids = ids[(ids >= 0) & (ids < off.shape[0] - 1)]
        ids = ids[off[ids + 1] > off[ids]] if ids.size else ids
        if ids.size == 0:
            return dist, rows
        tok = np.concatenate([self._tok[off[i]:off[i + 1]] for i in ids], axis=0)
        sub_off = np.concatenate([[0], np.cumsum(off[ids + 1] - off[ids])]).astype(np.int64)
        d, r = self._o.maxsim_topk(tok, sub_off, qtok, q_offsets, k)
        live = (np.diff(q_offsets) > 0)[:, None] & (r >= 0)      # a query without vectors: nothing (mi355dr_search_maxsim)
        dist[live], rows[live] = d[live], ids[np.maximum(r, 0)][live] + self.row_offset
        return dist, rows

    def maxsim_subset(self, *a, **kw):
        if self.calls is not None:
            self.calls["maxsim_subset"] += 1
        return super().maxsim_subset(*a, **kw)


def _same32(a, b):
    """two (dist, rows) results agree bit for bit (NaN positions, not payloads)"""
    (da, ra), (db, rb) = a, b
    assert np.array_equal(ra, rb)
    assert np.array_equal(np.isnan(da), np.isnan(db))
    ok = ~np.isnan(da)
    assert np.array_equal(np.ascontiguousarray(da, np.float32)[ok].view(np.uint32), np.ascontiguousarray(db, np.float32)[ok].view(np.uint32))


# ---- ShardedSearcher under gloo, world 2 ----------------------------------------------------------------------------------
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


N_DOCS, SPLIT, DIM = 401, 200, 16


def _sharded_case():
    rng = np.random.default_rng(123)
    docs = [rng.standard_normal((int(t), DIM)).astype(np.float32) for t in rng.integers(0, 9, size=N_DOCS)]
    docs[0] = docs[0][:0]               # a listed document without vectors
    docs[7] = docs[350] = rng.standard_normal((4, DIM)).astype(np.float32)   # an exact tie across the shard boundary
    qlens = [3, 4, 0, 6]
    qs = [rng.standard_normal((t, DIM)).astype(np.float32) for t in qlens]
    qs[1] = docs[7].copy()              # ... that ranks first for this query: the lower global id wins on every rank
    qtok = np.concatenate(qs, axis=0)
    qoff = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    both = np.concatenate([rng.choice(N_DOCS, size=120, replace=False), [7, 350, 0, -1, -1, N_DOCS, N_DOCS + 9, 7]])
    rng.shuffle(both)
    upper = np.arange(250, 330)         # leaves rank 0 with nothing
    return docs, qtok, qoff, both, upper


def _flat(docs):
    tok = np.concatenate(docs, axis=0).reshape(-1, DIM)
    return tok, np.concatenate([[0], np.cumsum([t.shape[0] for t in docs])]).astype(np.int64)


def _worker(rank: int, world: int, port: int, out_dir: str):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    from autorag_research_amd.sharded import ShardedSearcher
    from test_maxsim_subset_host import SPLIT, OracleMaxsimSubsetIndex, _flat, _sharded_case

    dist.init_process_group("gloo", rank=rank, world_size=world)
    docs, qtok, qoff, both, upper = _sharded_case()
    lo, hi = (0, SPLIT) if rank == 0 else (SPLIT, len(docs))
    s = ShardedSearcher(DIM, "cosine", index_factory=OracleMaxsimSubsetIndex)
    s.add_local_multivec(*_flat(docs[lo:hi]), lo)
    out = {}
    out["d_both"], out["r_both"] = s.search_maxsim_subset(qtok, qoff, 12, both)
    out["d_up"], out["r_up"] = s.search_maxsim_subset(qtok, qoff, 5, upper)
    out["d_big"], out["r_big"] = s.search_maxsim_subset(qtok, qoff, 300, both)     # k above the listed documents: NaN / -1 tail
    out["d_none"], out["r_none"] = s.search_maxsim_subset(qtok, qoff, 3, np.zeros(0, np.int64))
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_maxsim_subset_equals_unsharded(tmp_path, oracle):
    import torch.multiprocessing as mp

    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    docs, qtok, qoff, both, upper = _sharded_case()
    one = OracleMaxsimSubsetIndex(DIM)          # one index holding every document
    one.add_multivec(*_flat(docs))
    exp_both = one.search_maxsim_subset(qtok, qoff, 12, both)
    assert exp_both[1][1, :2].tolist() == [7, 350] and exp_both[0][1, 0] == exp_both[0][1, 1]
    assert (exp_both[1][2] == -1).all() and not (exp_both[1] == 0).any()      # the query / the document without vectors
    for o in (np.load(tmp_path / f"r{r}.npz") for r in range(world)):
        _same32((o["d_both"], o["r_both"]), exp_both)
        _same32((o["d_up"], o["r_up"]), one.search_maxsim_subset(qtok, qoff, 5, upper))
        assert (o["r_up"][[0, 1, 3]] >= 250).all()
        _same32((o["d_big"], o["r_big"]), one.search_maxsim_subset(qtok, qoff, 300, both))
        assert (o["r_big"][:, -1] == -1).all() and (o["r_none"] == -1).all() and np.isnan(o["d_none"]).all()


# ---- the service's `within=` in search_mode="multi" -------------------------------------------------------------------------
def _service(monkeypatch, index_cls):
    import autorag_research_amd.service as svc
    from autorag_research_amd.store import InMemoryStore

    monkeypatch.setattr(svc, "Mi355Index", index_cls)
    rng = np.random.default_rng(31)
    n, d, dm = 90, 24, 8
    C = rng.standard_normal((n, d)).astype(np.float32)
    docs = [rng.standard_normal((int(t), dm)).astype(np.float32) for t in rng.integers(1, 9, size=n)]
    docs[44] = docs[5].copy()                           # an exact tie: the earlier row first
    for i in (3, 13, 60):
        docs[i] = None
    ids = [f"c{i:03d}" for i in range(n)]
    store = InMemoryStore()
    store.set_chunks(ids, [f"text {i}" for i in range(n)], embedding=C, multivec=docs)
    Qm = [rng.standard_normal((t, dm)).astype(np.float32) for t in (2, 5, 1)]
    Qm[1] = docs[5].copy()
    store.add_queries(["q0", "q1", "q2"], contents=["a", "b", "c"], embedding=list(rng.standard_normal((3, d)).astype(np.float32)),
                      embeddings=Qm)
    return svc.Mi355RetrievalService(lambda: store)


KEYS = ["c005", "c003", "c044", "nope", "c013", "c071", "c005", "c030"]


def _answers(s):
    return [s.vector_search(["q0", "q1", "q2"], 3, "multi", within=KEYS), s.vector_search(["q1"], 50, "multi", within=KEYS),
            s.vector_search(["q1"], 5, "multi", within=["nope", "c003"]), s.vector_search(["q2"], 2, "multi", within=["c071"])]


def test_service_within_multi_same_dicts_through_both_paths(monkeypatch, oracle):
    calls = {"search_maxsim_subset": 0, "maxsim_subset": 0}
    monkeypatch.setattr(OracleMaxsimSubsetIndex, "calls", calls)
    new = _answers(_service(monkeypatch, OracleMaxsimSubsetIndex))
    assert calls == {"search_maxsim_subset": 3, "maxsim_subset": 0}    # one call per search; the list without a live key makes none
    assert not hasattr(OracleIndex, "search_maxsim_subset")            # the stand-in of the other tests keeps working without it
    old = _answers(_service(monkeypatch, OracleIndex))
    assert new == old
    assert [r["doc_id"] for r in new[0][1][:2]] == ["c005", "c044"] and new[0][1][0]["score"] == new[0][1][1]["score"]
    assert len(new[1][0]) == 4 and new[2] == [[]] and [r["doc_id"] for r in new[3][0]] == ["c071"]


def test_service_calls_the_new_method_once(monkeypatch, oracle):
    calls = {"search_maxsim_subset": 0, "maxsim_subset": 0}
    monkeypatch.setattr(OracleMaxsimSubsetIndex, "calls", calls)
    s = _service(monkeypatch, OracleMaxsimSubsetIndex)
    got = s.vector_search(["q0", "q1", "q2"], 3, "multi", within=KEYS)
    assert calls == {"search_maxsim_subset": 1, "maxsim_subset": 0} and all(len(g) == 3 for g in got)


# ---- the ABI symbols --------------------------------------------------------------------------------------------------------
def test_abi_symbols_declared_exported_bound(native_built):
    import ctypes

    from autorag_research_amd import _native

    header = (ROOT / "include" / "mi355dr.h").read_text()
    lib = ctypes.CDLL(str(native_built))
    for name in ("mi355dr_search_maxsim_subset", "mi355dr_search_maxsim_subset_device"):
        assert f"int {name}(" in header and name in _native.ABI_SYMBOLS and hasattr(lib, name)
        assert getattr(_native.load(), name).argtypes is not None
