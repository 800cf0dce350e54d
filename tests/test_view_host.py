"""CPU, world_size 2 over gloo: ShardedSearcher.view -- every rank passes the same lists, each keeps what falls in its shard, and
the unchanged search pipelines over the views give every rank the single-process oracle answer over the listed rows / documents.

The stand-in index is tests/helpers.OracleIndex with a `view` method of Mi355Index.view's contract: global ids in, the listed
rows that fall in this shard kept in ascending id order, results under the parent's global ids."""

import os
import socket
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

from helpers import OracleIndex  # noqa: E402


class ViewOracleIndex(OracleIndex):
    """OracleIndex + `view`: a stand-in of its own over the listed rows / documents, with the map back to the global ids"""

    is_view = False

    @staticmethod
    def _local(ids, offset, n):
        ids = np.unique(np.asarray([] if ids is None else ids, dtype=np.int64).reshape(-1)) - offset
        return ids[(ids >= 0) & (ids < n)]

    def view(self, row_ids=None, doc_ids=None):
        v = type(self)(self.dim, self.metric, self.device)
        v.is_view = True
        rows = self._local(row_ids, self.row_offset, len(self))
        v._rows, v._row_map = self._rows[rows], rows + self.row_offset
        docs = self._local(doc_ids, self.row_offset, self.n_docs())
        if docs.size:
            docs = docs[self._off[docs + 1] > self._off[docs]]
        if docs.size:
            v._tok = np.concatenate([self._tok[self._off[i]:self._off[i + 1]] for i in docs], axis=0)
            v._off = np.concatenate([[0], np.cumsum(self._off[docs + 1] - self._off[docs])]).astype(np.int64)
        v._doc_map = docs + self.row_offset
        return v

    def search(self, queries, k):
        d, r = super().search(queries, k)
        return (d, np.where(r >= 0, self._row_map[np.maximum(r, 0)], -1)) if self.is_view and len(self) else (d, r)

    def search_maxsim(self, qtok, q_offsets, k):
        if self.is_view and self._off is None:   # nothing listed falls in this shard
            B = len(q_offsets) - 1
            return np.full((B, k), np.nan, np.float32), np.full((B, k), -1, np.int64)
        d, r = super().search_maxsim(qtok, q_offsets, k)
        return (d, np.where(r >= 0, self._doc_map[np.maximum(r, 0)], -1)) if self.is_view else (d, r)

    def set_option(self, key, value):
        if self.is_view and key == "row_offset":
            raise ValueError("a view is read-only")
        super().set_option(key, value)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


N, D, B, K = 3001, 48, 9, 12


def _case():
    rng = np.random.default_rng(2718)
    C = rng.standard_normal((N, D)).astype(np.float32)
    C[5] = C[2900]        # a cross-shard exact tie, both rows listed: the lower global row wins
    C[17] = 0.0           # a listed row with a NaN distance
    Q = rng.standard_normal((B, D)).astype(np.float32)
    rows = np.unique(np.concatenate([rng.choice(N, size=700, replace=False), [5, 17, 2900]]))
    dirty = np.concatenate([rows, rows[::9], [-1, -1, N, N + 7, 2**40]])
    rng.shuffle(dirty)
    lens = rng.integers(0, 30, size=400)  # ragged, some docs without vectors
    lens[:40] = rng.integers(60, 90, size=40)
    tok = rng.standard_normal((int(lens.sum()), 24)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    qtok = rng.standard_normal((5 + 11, 24)).astype(np.float32)
    docs = rng.choice(400, size=150, replace=False)
    return C, Q, rows, dirty, tok, off, qtok, np.array([0, 5, 16], dtype=np.int32), docs


def _worker(rank: int, world: int, port: int, out_dir: str):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist

    from autorag_research_amd.sharded import ShardedSearcher, shard_bounds, shard_bounds_by_tokens
    from test_view_host import ViewOracleIndex, _case

    dist.init_process_group("gloo", rank=rank, world_size=world)
    C, Q, rows, dirty, tok, off, qtok, qoff, docs = _case()
    lo, hi = shard_bounds(N, world, rank, granule=250)
    s = ShardedSearcher(D, "cosine", index_factory=ViewOracleIndex)
    s.add_local(C[lo:hi], lo)
    sv = s.view(row_ids=dirty)
    assert sv.index.is_view and sv.index is not s.index and sv.group is s.group and sv.world == world
    assert len(sv.index) == int(((rows >= lo) & (rows < hi)).sum())
    d1, r1 = sv.search(Q, K)
    d2, r2 = sv.search(Q, K, block=4)    # the overlapped pipeline: 3 blocks
    assert sv.overlapped_blocks == 2 and s.overlapped_blocks == 0
    assert np.array_equal(r1, r2) and np.array_equal(d1.view(np.uint64), d2.view(np.uint64))
    few = s.view(row_ids=[1, 2, N - 1])   # one rank holds two rows, the other one: k above both
    df, rf = few.search(Q[:2], 5)
    full_d, full_r = s.search(Q, K)       # the parent searcher still answers over every row
    dlo, dhi = shard_bounds_by_tokens(off, world, rank)
    m = ShardedSearcher(tok.shape[1], "cosine", index_factory=ViewOracleIndex)
    m.add_local_multivec(tok[off[dlo]:off[dhi]], off[dlo:dhi + 1] - off[dlo], dlo)
    mv = m.view(doc_ids=np.concatenate([docs, docs[:10], [-1, 400, 999]]))
    md, mr = mv.search_maxsim(qtok, qoff, 9)
    for x in (sv, few, mv):
        x.close()
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), d=d1, r=r1, df=df, rf=rf, fd=full_d, fr=full_r, md=md, mr=mr)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_view_equals_single_process_oracle(tmp_path, oracle):
    import torch.multiprocessing as mp

    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    C, Q, rows, dirty, tok, off, qtok, qoff, docs = _case()
    d, r = oracle.topk_search(C[rows], Q, K)
    want_r = np.where(r >= 0, rows[np.maximum(r, 0)], -1)
    assert (want_r[:, 0] >= 0).all() and 5 in rows and 2900 in rows
    few = np.array([1, 2, N - 1])
    dfw, rfw = oracle.topk_search(C[few], Q[:2], 5)
    full_d, full_r = oracle.topk_search(C, Q, K)
    kept = np.array(sorted(i for i in set(docs.tolist()) if off[i + 1] > off[i]), np.int64)
    assert 0 < kept.size < docs.size
    sub_tok = np.concatenate([tok[off[i]:off[i + 1]] for i in kept], axis=0)
    sub_off = np.concatenate([[0], np.cumsum(off[kept + 1] - off[kept])]).astype(np.int64)
    md, mr = oracle.maxsim_topk(sub_tok, sub_off, qtok, qoff, 9)
    for rank in range(world):
        o = np.load(tmp_path / f"r{rank}.npz")
        assert np.array_equal(o["r"], want_r) and np.array_equal(o["d"], d, equal_nan=True)
        assert np.array_equal(o["rf"], np.where(rfw >= 0, few[np.maximum(rfw, 0)], -1)) and (o["rf"][:, 3:] == -1).all()
        assert np.array_equal(o["df"], dfw, equal_nan=True)
        assert np.array_equal(o["fr"], full_r) and np.array_equal(o["fd"], full_d, equal_nan=True)
        assert np.array_equal(o["mr"], kept[mr]) and np.array_equal(o["md"].view(np.uint32), md.view(np.uint32))


def test_view_shares_the_group_and_closes_alone():
    """no process group: ShardedSearcher.view copies the searcher's settings, swaps the index, and close() releases the view only"""
    from autorag_research_amd.sharded import ShardedSearcher

    closed = []

    class Idx(ViewOracleIndex):
        def close(self):
            closed.append(self.is_view)

    s = ShardedSearcher(8, "cosine", index_factory=Idx)
    s.add_local(np.eye(8, dtype=np.float32), 100)
    v = s.view(row_ids=[103, 101, 101, 5, 999])
    assert isinstance(v, ShardedSearcher) and v.index.is_view and not s.index.is_view
    assert (v.world, v.rank, v.group, v.row_offset, v.force_pipeline) == (s.world, s.rank, s.group, 100, False)
    d, r = v.search(np.eye(8, dtype=np.float32)[1], 3)
    assert r.tolist() == [[101, 103, -1]] and d[0, 0] == 0.0 and np.isnan(d[0, 2])
    v.close()
    assert closed == [True]
    assert s.search(np.eye(8, dtype=np.float32)[3], 1)[1].tolist() == [[103]]
