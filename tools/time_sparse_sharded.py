"""Time `search_bm25_sharded_device` on one GPU at world size 1, over the library's RCCL communicator, next to the local
`search_bm25_device` on the same handle in the same run.

    python tools/time_sparse_sharded.py --docs 1000000 --vocab 100000 --doc-len 60 --queries 1024 --query-terms 8 --repeats 7

The corpus and the queries are tools/time_bm25.py's (Zipf tokens, a query is tokens of one document).  A one-GPU box cannot show
what sharding buys: at world 1 the sharded form does the local work plus the statistics gather, the packed list, its gather and
the merge.  This tool prices those pieces; no threshold is set on them.

Legs, one block of `--queries` queries per call, host clock around calls that are complete on return, one warm-up of each leg,
the legs alternating inside every repeat, best and all values kept:
    local_a, local_b   search_bm25_device, twice per repeat: two series whose difference is the run-to-run spread of the call
    sharded            search_bm25_sharded_device (must equal the local result bit for bit)
    empty_local        search_bm25_subset(device_out=True) with an EMPTY list: the call frame without any scoring
    empty_sharded      search_bm25_subset_sharded with the same list: the same plus statistics gather, list gather, merge
    empty_local_w / empty_sharded_w   the weighted forms of the two (the BM25 terms with unit weights): the statistics carry no df
    merge              merge_topk_packed_device of one rank's packed [2, B, k] block, and a synchronize
The tool runs ONE build.  Whether the local call kept the parent commit's time is shown by tools/time_bm25.py (same corpus and
queries, `--ref-queries 0`) run on a checkout of the parent, on this tree, and on the parent again on the same box: the
parent's two runs give the run-to-run spread this tree's figure is held against (profiles/sparse_sharded_timing.txt records
the three).  local_a / local_b here are the spread inside one process only.
Derived (ms per block, and as a share of the sharded call).  The statistics gather, the list gather and the merge are NOT
timed one by one -- the library has no clock inside a call --: the merge is timed alone, the df-dependent part of the
statistics path by difference, and the two gathers' fixed cost (the list gather and the 16-byte statistics gather that every
call makes) stay lumped in `gathers_fixed`:
    exchange           empty_sharded - empty_local            statistics gather + list gather + merge, no scoring
    statistics_df      exchange - (empty_sharded_w - empty_local_w)   what the T df words cost: union, payload, fold, weights
    merge              as measured
    gathers_fixed      (empty_sharded_w - empty_local_w) - merge      the list gather and the 16-byte statistics gather
One JSON line."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--doc-len", type=int, default=60)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--query-terms", type=int, default=8)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from time_bm25 import doc_queries, zipf_corpus

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n, B, k = a.docs, a.queries, a.k
    terms, offsets, lengths = zipf_corpus(rng, n, a.vocab, a.doc_len)
    queries = doc_queries(rng, terms, offsets, lengths, B, a.query_terms)
    distinct = [sorted(set(q)) for q in queries]
    w_terms = [t for q in distinct for t in q]
    w_off = np.concatenate([[0], np.cumsum([len(q) for q in distinct])])
    w_weights = np.ones(len(w_terms))
    none = np.empty(0, dtype=np.int64)

    with Mi355Index(8) as idx:
        idx.add_sparse(terms, offsets)
        idx.comm_init(0, 1, Mi355Index.comm_unique_id())
        od, orr = idx.dev_alloc(B * k * 8), idx.dev_alloc(B * k * 8)
        packed = idx.dev_alloc(2 * B * k * 8)
        try:
            def merge():
                idx.merge_topk_packed_device(packed, 1, B, k, od, orr)
                idx.synchronize()

            legs = {
                "local_a": lambda: idx.search_bm25_device(queries, k, od, orr),
                "sharded": lambda: idx.search_bm25_sharded_device(queries, k, od, orr),
                "local_b": lambda: idx.search_bm25_device(queries, k, od, orr),
                # (the four empty-list legs go through the same allocate-call-download wrapper on both sides)
                "empty_local": lambda: idx.search_bm25_subset(queries, k, none, device_out=True),
                "empty_sharded": lambda: idx.search_bm25_subset_sharded(queries, k, none),
                "empty_local_w": lambda: idx.search_sparse_subset(w_terms, w_weights, w_off, k, none, device_out=True),
                "empty_sharded_w": lambda: idx.search_sparse_subset_sharded(w_terms, w_weights, w_off, k, none),
                "merge": merge,
            }
            got = {}
            times = {name: [] for name in legs}
            idx.search_bm25_device(queries[:1], k, od, orr)         # the layout build
            for rep in range(a.repeats + 1):                        # (repeat 0: warm-up of every leg, not kept)
                for name, fn in legs.items():
                    if name == "merge":                             # a valid packed block: this rank's own list
                        idx.search_bm25_device(queries, k, od, orr)
                        idx.pack_topk_device(od, orr, B, k, packed)
                        idx.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    if rep:
                        times[name].append((time.perf_counter() - t0) * 1e3)
                    if rep == a.repeats and name in ("local_a", "sharded"):
                        d, r = np.empty((B, k)), np.empty((B, k), dtype=np.int64)
                        idx.dev_download(od, d)
                        idx.dev_download(orr, r)
                        got[name] = (d, r)
            gather = idx.stat("shard_gather_bytes")
            calls = idx.stat("sharded_sparse_searches")
        finally:
            for p in (od, orr, packed):
                idx.dev_free(p)
    best = {name: min(t) for name, t in times.items()}
    exchange = best["empty_sharded"] - best["empty_local"]
    fixed = best["empty_sharded_w"] - best["empty_local_w"]
    pieces = {"exchange": exchange, "statistics_df": exchange - fixed, "merge": best["merge"], "gathers_fixed": fixed - best["merge"]}
    same = bool(np.array_equal(got["local_a"][1], got["sharded"][1])
                and np.array_equal(got["local_a"][0].view(np.uint64), got["sharded"][0].view(np.uint64)))
    print(json.dumps({
        "docs": n, "vocab": a.vocab, "tokens": int(offsets[-1]), "queries": B, "query_terms": a.query_terms, "k": k,
        "repeats": a.repeats, "world": 1, "distinct_query_terms": len(set(w_terms)),
        "ms_per_block_best": {name: round(t, 3) for name, t in best.items()},
        "ms_per_block_all": {name: [round(x, 3) for x in t] for name, t in times.items()},
        "local_spread_ms": round(abs(best["local_a"] - best["local_b"]), 3),
        "sharded_over_local": round(best["sharded"] / min(best["local_a"], best["local_b"]), 3),
        "pieces_ms": {name: round(t, 3) for name, t in pieces.items()},
        "pieces_share_of_sharded": {name: round(t / best["sharded"], 4) for name, t in pieces.items()},
        "shard_gather_bytes_per_sharded_call": int(gather // max(calls, 1)),
        "sharded_equals_local": same,
    }))


if __name__ == "__main__":
    main()
