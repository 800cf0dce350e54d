"""GPU, TWO ranks on ONE MI355X over gloo (the form of tests/test_gpu_world2.py): the sparse store cut unevenly over two
ranks, searched through `ShardedSearcher` -- the library's sharded forms over `mi355dr_comm_init_custom` with the gloo host-hop
all-gather as the transport.  Every rank's result == tests/sparse_ref.py / sparse_subset_ref.py over the WHOLE corpus == one
whole `Mi355Index` on the same GPU: ids equal, distance bits equal, NaN / -1 tails equal.  The two shards' document lengths are
drawn differently, so a shard that scored with its own statistics would fail.  One pair of processes, every case inside the
child."""

import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CHILD_TIMEOUT_S = 300

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
import sparse_ref, sparse_subset_ref

rank, world = int(os.environ["RANK"]), 2
dist.init_process_group("gloo", rank=rank, world_size=world)
torch.cuda.set_device(0)

N, CUT, VOCAB = 6000, 2500, 300
ONLY_1, NOWHERE, TWIN_TERM, RARE = 900, 950, 901, 902
TWIN_A, TWIN_B = 100, 2600


def corpus():
    rng = np.random.default_rng(77)
    docs = []
    for i in range(N):
        n = int(rng.integers(1, 21)) if i < CUT else int(rng.integers(10, 61))    # short documents on rank 0, long ones on rank 1
        docs.append(rng.integers(0, VOCAB, size=n).tolist())
    for i in range(7, N, 501):
        docs[i] = []                                                             # documents without tokens on both shards
    for i in range(CUT + 3, N, 97):
        docs[i] = docs[i] + [ONLY_1]
    for i in (40, 1200, 2400) + tuple(range(CUT + 10, CUT + 10 + 30 * 50, 50)):
        docs[i] = docs[i] + [RARE]                                               # 3 on rank 0, 30 on rank 1
    docs[TWIN_A] = [5, 5, 9, TWIN_TERM]
    docs[TWIN_B] = [5, 5, 9, TWIN_TERM]                                          # identical documents, one per shard
    return docs


def token_queries():
    rng = np.random.default_rng(78)
    qs = [rng.integers(0, VOCAB + 10, size=int(rng.integers(1, 7))).tolist() for _ in range(20)]
    return qs + [[], [ONLY_1], [NOWHERE], [NOWHERE, 3, ONLY_1], [TWIN_TERM, 5], [RARE], [-2, 1 << 21]]


def weighted_queries():
    rng = np.random.default_rng(79)
    terms, weights, off = [], [], [0]
    for _ in range(12):
        t = rng.choice(VOCAB + 5, size=int(rng.integers(0, 6)), replace=False)
        terms += t.tolist()
        weights += rng.uniform(-1.0, 2.0, size=len(t)).tolist()
        off.append(len(terms))
    terms += [TWIN_TERM, 5, ONLY_1]
    weights += [1.0, 0.5, -0.25]
    off.append(len(terms))
    return terms, weights, off


def as_pairs(wq):
    t, w, off = wq
    return [(t[off[i]:off[i + 1]], w[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def same(got, exp, what):
    assert got[0].shape == exp[0].shape, what
    assert np.array_equal(got[1], exp[1]), (what, np.argwhere(got[1] != exp[1])[:5])
    assert np.array_equal(np.ascontiguousarray(got[0]).view(np.int64), np.ascontiguousarray(exp[0]).view(np.int64)), what


def same_scores(got, exp, what):
    assert got.shape == exp.shape and np.array_equal(np.isnan(got), np.isnan(exp)), what
    assert np.array_equal(got[~np.isnan(got)].view(np.int64), exp[~np.isnan(exp)].view(np.int64)), what


def make(docs, lo, hi):
    s = ShardedSearcher(8, "cosine", device=0)
    s.index.set_option("sparse_tile_docs", 256)
    s.index.set_option("sparse_subset_pairs_max", 64)
    s.add_local_sparse(docs[lo:hi], lo)
    whole = pkg.Mi355Index(8)
    whole.set_option("sparse_tile_docs", 256)
    whole.set_option("sparse_subset_pairs_max", 64)
    whole.add_sparse(docs)
    return s, whole


def check_all(s, whole, docs, tag):
    ref = sparse_ref.SparseCorpus(docs)
    tq, wq = token_queries(), weighted_queries()
    rng = np.random.default_rng(80)
    short = np.concatenate([rng.integers(0, N, size=40), [-1, N, N + 9, TWIN_A, TWIN_B, TWIN_B]])
    long_ = rng.integers(-20, N + 20, size=700)
    for ids in (short, long_):
        assert (ids[(ids >= 0) & (ids < N)] < CUT).any() and (ids >= CUT).any()   # the list spans both shards
    for k in (10, 100):
        exp = sparse_ref.search_bm25(ref, tq, k)
        same(s.search_bm25(tq, k), exp, (tag, "bm25 vs reference", k))
        same(whole.search_bm25(tq, k), exp, (tag, "whole index vs reference", k))
        exp = sparse_ref.search_weighted(ref, as_pairs(wq), k, 0.9, 0.4)
        same(s.search_sparse(*wq, k, 0.9, 0.4), exp, (tag, "weighted vs reference", k))
        same(whole.search_sparse(*wq, k, 0.9, 0.4), exp, (tag, "whole index weighted", k))
        for ids in (short, long_):
            exp = sparse_subset_ref.search_bm25_subset(ref, tq, k, ids)
            same(s.search_bm25_subset(tq, k, ids), exp, (tag, "bm25 subset", k, len(ids)))
            same(whole.search_bm25_subset(tq, k, ids), exp, (tag, "whole bm25 subset", k, len(ids)))
            exp = sparse_subset_ref.search_weighted_subset(ref, as_pairs(wq), k, ids)
            same(s.search_sparse_subset(*wq, k, ids), exp, (tag, "weighted subset", k, len(ids)))
    pool = rng.integers(-3, N + 3, size=(len(tq), 11))
    pool[:, 4], pool[:, 6] = pool[:, 3], -1                                       # a duplicate and a -1 in every row
    pool[-3, :3] = [TWIN_B, TWIN_A, TWIN_B]
    exp = sparse_subset_ref.score_bm25_subset(ref, tq, pool)
    assert (~np.isnan(exp)).sum() > 10
    same_scores(s.score_bm25_subset(tq, pool), exp, (tag, "bm25 scores"))
    pw = pool[:len(wq[2]) - 1]
    same_scores(s.score_sparse_subset(*wq, pw, 0.9, 0.4), sparse_subset_ref.score_weighted_subset(ref, as_pairs(wq), pw, 0.9, 0.4),
                (tag, "weighted scores"))
    return ref


docs = corpus()
lo, hi = (0, CUT) if rank == 0 else (CUT, N)
s, whole = make(docs, lo, hi)

# the fixture can tell global statistics from local ones, and holds the cases it is meant to hold
ref = sparse_ref.SparseCorpus(docs)
parts = [sparse_ref.SparseCorpus(docs[:CUT]), sparse_ref.SparseCorpus(docs[CUT:])]
avgdl = ref.total_len / ref.n_live
for p in parts:
    assert abs(p.total_len / p.n_live - avgdl) > 3.0
assert parts[0].df(ONLY_1) == 0 and parts[1].df(ONLY_1) > 10 and ref.df(NOWHERE) == 0
assert parts[0].df(RARE) == 3 and parts[1].df(RARE) == 30                        # fewer than k = 10 matches on shard 0
d, r = sparse_ref.search_bm25(ref, [[TWIN_TERM, 5]], 10)
assert r[0, :2].tolist() == [TWIN_A, TWIN_B] and d[0, 0] == d[0, 1]              # the lower global id first

s.index.reset_stats()
check_all(s, whole, docs, "fresh")
got = s.search_bm25([[TWIN_TERM, 5]], 10)
assert got[1][0, :2].tolist() == [TWIN_A, TWIN_B]
assert s.index.comm_world() == 2 and s.index.stat("sharded_sparse_searches") > 0 and s.index.stat("sharded_sparse_scores") == 2
assert s.index.stat("shard_gather_bytes") > 0 and s.index.stat("sparse_searches") == 0

# rank 1 replaces one document and removes another; BOTH ranks search again
new_doc = [ONLY_1, 3, 3, 4, NOWHERE]
if rank == 1:
    s.set_local_sparse([3000], [new_doc])
    s.remove_local_sparse([4000])
else:
    for bad in ([3000], [CUT]):
        try:
            s.set_local_sparse(bad, [new_doc])
        except ValueError:
            pass
        else:
            raise AssertionError("rank 0 accepted a document id of rank 1")
whole.set_sparse([3000], [new_doc])
whole.remove_sparse([4000])
docs2 = list(docs)
docs2[3000], docs2[4000] = new_doc, []
ref2 = check_all(s, whole, docs2, "mutated")
assert ref2.df(NOWHERE) == 1 and ref2.n_live == ref.n_live - 1
s.close()
whole.close()

# a second, small store: rank 0 holds only documents without tokens
rng = np.random.default_rng(81)
small = [[] for _ in range(3)] + [rng.integers(0, 20, size=int(rng.integers(1, 9))).tolist() for _ in range(50)]
lo, hi = (0, 3) if rank == 0 else (3, len(small))
s2 = ShardedSearcher(8, "cosine", device=0)
s2.add_local_sparse(small[lo:hi], lo)
ref3 = sparse_ref.SparseCorpus(small)
tq = [[1, 2, 3], [19], [], [25]]
same(s2.search_bm25(tq, 10), sparse_ref.search_bm25(ref3, tq, 10), "small store")
pool = np.array([[0, 1, 5, 52], [2, 3, 4, -1], [7, 8, 9, 10], [0, 0, 0, 0]])
same_scores(s2.score_bm25_subset(tq, pool), sparse_subset_ref.score_bm25_subset(ref3, tq, pool), "small store scores")
assert s2.index.live_sparse() == (0 if rank == 0 else 50)
s2.close()
dist.barrier()
dist.destroy_process_group()
print("SPARSE2_OK", rank)
"""

# what a lost rendezvous looks like in a child's stderr: the only failure that earns a second attempt
_RENDEZVOUS = ("DistNetworkError", "DistStoreError", "Connection refused", "Address already in use", "EADDRINUSE",
               "Connection reset by peer", "failed to connect")


def _run_pair():
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
            outs.append(p.communicate(timeout=CHILD_TIMEOUT_S))
        except subprocess.TimeoutExpired:
            for pp in procs:
                pp.kill()
            raise
    bad = [rank for rank, (p, (so, _)) in enumerate(zip(procs, outs)) if p.returncode != 0 or f"SPARSE2_OK {rank}" not in so]
    report = "\n".join(f"rank {rank}: exit code {procs[rank].returncode}\n--- stdout\n{outs[rank][0][-800:]}\n--- stderr\n"
                       f"{outs[rank][1][-3500:]}" for rank in bad)
    # a rank that died of a signal (a fault, an abort) is never a lost rendezvous
    lost = bool(bad) and all(procs[rank].returncode > 0 for rank in bad) and any(t in report for t in _RENDEZVOUS) \
        and "AssertionError" not in report and "NativeError" not in report
    return report, lost


def test_two_uneven_shards_equal_the_whole_corpus(native_built):
    report, lost = _run_pair()
    if report and lost:
        report, _ = _run_pair()            # one more attempt, for a lost rendezvous only
    if report:
        pytest.fail(report)
