"""Time `Mi355Index.search_subset_device` on one GPU next to the exact scan over the whole index (`path = scan`).

    python tools/time_subset.py --rows 1000000 --dim 768 --queries 1024 --k 10 --repeats 5

Timed with the host clock around calls that are complete on return (queries and outputs stay in device memory; a subset
call's time includes sorting and uploading its id list), after one warm-up of every shape; the variants alternate inside
every repeat, best and all values are kept:
  subset_<m>    search_subset over m rows drawn at random (m = 10 000, 100 000) and over every row (m = rows)
  scan          search, path = scan: the LDS-DMA form k_scan32 when dim % 32 == 0
  scan_generic  the same with scan_dma = 0: k_scan, the form k_scan_ids is built from
Per variant: ms per call and ns per listed row per 32-query group (ms / (m x ceil(queries / 32))).  Prints one JSON line.
The corpus is Gaussian: one generated chunk, its columns rotated by the chunk number."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n, d, B, k = a.rows, a.dim, a.queries, a.k
    chunk = min(n, 250_000)
    base = rng.standard_normal((chunk, d), dtype=np.float32)
    Q = rng.standard_normal((B, d), dtype=np.float32)
    lists = {m: np.sort(rng.choice(n, m, replace=False)) for m in (10_000, 100_000) if m < n}
    lists[n] = np.arange(n, dtype=np.int64)
    groups = (B + 31) // 32

    with Mi355Index(d) as idx:
        for c, r0 in enumerate(range(0, n, chunk)):
            idx.add(np.roll(base, c, axis=1)[:min(chunk, n - r0)])
        pq, od, orr = idx.dev_alloc(Q.nbytes), idx.dev_alloc(B * k * 8), idx.dev_alloc(B * k * 8)
        idx.dev_upload(pq, Q)

        def scan(dma: int):
            idx.set_option("path", "scan")
            idx.set_option("scan_dma", dma)
            idx.search_device(pq, B, k, od, orr)
            idx.set_option("path", "auto")
            idx.set_option("scan_dma", 1)

        variants = {f"subset_{m}": (m, lambda ids=ids: idx.search_subset_device(pq, B, k, ids, od, orr))
                    for m, ids in lists.items()}
        variants["scan"] = (n, lambda: scan(1))
        variants["scan_generic"] = (n, lambda: scan(0))
        times = {name: [] for name in variants}
        for rep in range(a.repeats + 1):                          # (repeat 0: warm-up of every shape, not kept)
            for name, (_, fn) in variants.items():
                t0 = time.perf_counter()
                fn()
                if rep:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        idx.reset_stats()
        variants[f"subset_{n}"][1]()
        out = {"rows": n, "dim": d, "queries": B, "k": k, "repeats": a.repeats,
               "subset_rerun_queries_full_list": idx.stat("subset_rerun_queries")}
        for name, (m, _) in variants.items():
            best = min(times[name])
            out[name] = {"m": m, "ms_best": round(best, 3), "ms_all": [round(t, 3) for t in times[name]],
                         "ns_per_row_per_group": round(best * 1e6 / (m * groups), 4)}
        out["ratio_full_list_to_scan"] = round(out[f"subset_{n}"]["ms_best"] / out["scan"]["ms_best"], 3)
        out["ratio_full_list_to_scan_generic"] = round(out[f"subset_{n}"]["ms_best"] / out["scan_generic"]["ms_best"], 3)
        # the three ways to scan every row agree (ids and distance bits)
        res = []
        for name in (f"subset_{n}", "scan", "scan_generic"):
            variants[name][1]()
            gd, gr = np.empty((B, k)), np.empty((B, k), dtype=np.int64)
            idx.dev_download(od, gd)
            idx.dev_download(orr, gr)
            res.append((gd.view(np.uint64).copy(), gr))
        out["results_agree"] = all(np.array_equal(res[0][0], r[0]) and np.array_equal(res[0][1], r[1]) for r in res[1:])
        for p in (pq, od, orr):
            idx.dev_free(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
