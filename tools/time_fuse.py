"""Time what a hybrid page costs AFTER its two searches, on the host and on the device, on one GPU.

    python tools/time_fuse.py --repeats 7

Both legs' [B, fetch_k] lists are synthetic (a dense leg: cosine distances and index rows behind a non-identity map; a BM25
leg: negative distances and table positions; `--shared` of each query's BM25 documents are in its dense list too) and are in
HBM and in host memory before the clock starts, as the searches' two forms would leave them.  Per shape (B x fetch_k, top_k =
fetch_k / 2) and method (rrf, mm):
  host     the path of `_Mi355HybridBase._retrieve_block` today: two `_results_from_block`, then `rrf_fuse` / `cc_fuse` per query
  device   `Mi355RetrievalService.fuse_device_lists`: one fusion launch, one [B, top_k] download, the result dicts
  kernel   the fusion launch alone, between two events on the handle's stream
Host clock around work that is complete on return (events for `kernel`), one warm-up of every variant, the variants alternate
inside every repeat, medians reported.  Also checks that host and device return the same dicts, bit for bit.  Prints one JSON
line per shape and method."""

from __future__ import annotations

import argparse
import json
import statistics
import struct
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def make_page(rng, B, fetch_k, n_docs, shared):
    """(dense distances, dense rows, row -> position map, BM25 distances, BM25 positions)"""
    row_pos = np.delete(np.arange(n_docs, dtype=np.int64), np.arange(0, n_docs, 97))   # every 97th chunk has no embedding
    d_dist = np.sort(rng.random((B, fetch_k)) * 0.6 + 0.2, axis=1)
    s_dist = np.sort(-rng.random((B, fetch_k)) * 25.0, axis=1)
    d_rows = np.empty((B, fetch_k), dtype=np.int64)
    s_pos = np.empty((B, fetch_k), dtype=np.int64)
    n_shared = int(round(shared * fetch_k))
    for q in range(B):
        d_rows[q] = rng.choice(row_pos.shape[0], fetch_k, replace=False)
        mine = row_pos[d_rows[q]]
        others = np.setdiff1d(rng.choice(n_docs, 2 * fetch_k, replace=False), mine)[:fetch_k - n_shared]
        s_pos[q] = rng.permutation(np.concatenate([rng.choice(mine, n_shared, replace=False), others]))
    return d_dist, d_rows, row_pos, s_dist, s_pos


def bits(page):
    return [[(r["doc_id"], struct.pack("<d", r["score"])) for r in res] for res in page]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--fetch-ks", type=int, nargs="+", default=[20, 200, 1024])
    ap.add_argument("--methods", nargs="+", default=["rrf", "mm"])
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--shared", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index
    from autorag_research_amd.hybrid import cc_fuse, rrf_fuse
    from autorag_research_amd.service import DeviceLists, Mi355RetrievalService, _DevScratch
    from autorag_research_amd.store import ChunkTable

    rng = np.random.default_rng(a.seed)
    table = ChunkTable(ids=[10 * i + 3 for i in range(a.docs)], contents=[f"chunk {i}" for i in range(a.docs)])
    identity = np.arange(a.docs)
    build = Mi355RetrievalService._results_from_block
    with Mi355Index(8) as ix:
        scratch = _DevScratch()
        try:
            for B in a.batches:
                for fetch_k in a.fetch_ks:
                    top_k = max(fetch_k // 2, 1)
                    d_dist, d_rows, row_pos, s_dist, s_pos = make_page(rng, B, fetch_k, a.docs, a.shared)
                    ptrs = {}
                    for name, arr in (("d_dist", d_dist), ("d_rows", d_rows), ("map", row_pos), ("s_dist", s_dist), ("s_pos", s_pos)):
                        ptrs[name] = scratch.take(ix, name, arr.nbytes)
                        ix.dev_upload(ptrs[name], arr)
                    dense = DeviceLists(ix, scratch, ptrs["d_dist"], ptrs["d_rows"], B, fetch_k, "one_minus", ptrs["map"], row_pos.shape[0])
                    lex = DeviceLists(ix, scratch, ptrs["s_dist"], ptrs["s_pos"], B, fetch_k, "negate", 0, 0)
                    out_v = scratch.take(ix, "kernel_v", B * top_k * 8)
                    out_i = scratch.take(ix, "kernel_i", B * top_k * 8)
                    for method in a.methods:
                        spec = {"method": "rrf", "rrf_k": 60, "fetch_k": fetch_k} if method == "rrf" else {"method": method, "weight": 0.5}

                        def host():
                            p1 = build(table, row_pos, d_rows, 1.0 - d_dist, True)
                            p2 = build(table, identity, s_pos, -s_dist, True)
                            if method == "rrf":
                                return [rrf_fuse(x, y, 60, top_k, fetch_k) for x, y in zip(p1, p2)]
                            return [cc_fuse(x, y, 0.5, top_k, method) for x, y in zip(p1, p2)]

                        def device():
                            return Mi355RetrievalService.fuse_device_lists(dense, lex, table, top_k, **spec)

                        def kernel():
                            ix.timer_start()
                            ix.fuse_lists_device(dense.dist_ptr, dense.ids_ptr, fetch_k, lex.dist_ptr, lex.ids_ptr, fetch_k, B, top_k,
                                                 out_v, out_i, None, modes=("one_minus", "negate"), map1_ptr=dense.map_ptr,
                                                 map1_len=dense.map_len, **spec)
                            return ix.timer_stop()

                        variants = {"host": host, "device": device, "kernel": kernel}
                        times = {name: [] for name in variants}
                        last = {}
                        for rep in range(a.repeats + 1):          # (repeat 0: warm-up of every variant, not kept)
                            for name, fn in variants.items():
                                t0 = time.perf_counter()
                                last[name] = fn()
                                ms = (time.perf_counter() - t0) * 1e3
                                if rep:
                                    times[name].append(last[name] if name == "kernel" else ms)
                        out = {"B": B, "fetch_k": fetch_k, "top_k": top_k, "method": method, "shared": a.shared, "repeats": a.repeats}
                        for name in variants:
                            out[f"{name}_ms"] = round(statistics.median(times[name]), 3)
                            out[f"{name}_ms_min_max"] = [round(min(times[name]), 3), round(max(times[name]), 3)]
                        out["host_over_device"] = round(out["host_ms"] / out["device_ms"], 2)
                        out["same_bits"] = bits(last["host"]) == bits(last["device"])
                        print(json.dumps(out), flush=True)
        finally:
            scratch.release(ix)


if __name__ == "__main__":
    main()
