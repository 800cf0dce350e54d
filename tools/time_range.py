"""Time `Mi355Index.search_range` on one GPU next to the ordinary search at k = max_results, in the same run on the same index.

    python tools/time_range.py --rows 1000000 --dim 768 --queries 1024 --repeats 5 [--chunk-rows 131072]

Radii are taken from the k-th distances of one ordinary search at k = 1000, so that about 10, 100 and 1 000 rows per query are
in range.  For max_results = 10 and 100 and each of the three radii the variants `search_range(Q, radius, m)` and
`search(Q, m)` alternate inside every repeat; timed with the host clock around calls that are complete on return (host
buffers both ways), after one warm-up of every variant; best and all values are kept.  Every range result is checked against
the identity of include/mi355dr.h: the search at k = m with the entries above the radius blanked, and the counts against the
search at k = 1000.  Prints one JSON line per (max_results, radius) pair and one summary line.
The corpus is Gaussian: one generated chunk, its columns rotated by the chunk number."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

RANGE_STATS = ["range_candidates", "range_rescored", "range_redo_chunks", "range_fallback_queries", "range_in_range"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--path", default="auto")
    ap.add_argument("--chunk-rows", type=int, default=0, help="option range_chunk_rows (0: the library's default)")
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n, d, B = a.rows, a.dim, a.queries
    chunk = min(n, 250_000)
    base = rng.standard_normal((chunk, d), dtype=np.float32)
    Q = rng.standard_normal((B, d), dtype=np.float32)
    deep = 1000
    summary = {}
    with Mi355Index(d) as idx:
        for c, r0 in enumerate(range(0, n, chunk)):
            idx.add(np.roll(base, c, axis=1)[:min(chunk, n - r0)])
        idx.set_option("path", a.path)
        if a.chunk_rows:
            idx.set_option("range_chunk_rows", a.chunk_rows)
        dist_deep, _ = idx.search(Q, deep)
        for m in (10, 100):
            for in_range in (10, 100, 1000):
                radius = np.ascontiguousarray(dist_deep[:, in_range - 1])
                variants = {"search_range": lambda: idx.search_range(Q, radius, m), "search": lambda: idx.search(Q, m)}
                times = {name: [] for name in variants}
                last = {}
                for rep in range(a.repeats + 1):                  # (repeat 0: warm-up of every variant, not kept)
                    for name, fn in variants.items():
                        if rep == a.repeats:
                            idx.reset_stats()
                        t0 = time.perf_counter()
                        last[name] = fn()
                        if rep:
                            times[name].append((time.perf_counter() - t0) * 1e3)
                        if rep == a.repeats and name == "search_range":
                            stats = {key: idx.stat(key) for key in RANGE_STATS}
                (gd, gr, gc), (sd, sr) = last["search_range"], last["search"]
                with np.errstate(invalid="ignore"):
                    out_of_range = np.isnan(sd) | (sd > radius[:, None])
                ok = ~out_of_range
                same = bool(np.array_equal(gr, np.where(out_of_range, -1, sr)) and np.array_equal(np.isnan(gd), out_of_range)
                            and np.array_equal(gd[ok].view(np.uint64), sd[ok].view(np.uint64)))
                with np.errstate(invalid="ignore"):
                    counts_ok = bool(np.array_equal(gc, (dist_deep <= radius[:, None]).sum(axis=1)))
                out = {"rows": n, "dim": d, "queries": B, "max_results": m, "in_range_per_query": round(float(gc.mean()), 2),
                       "repeats": a.repeats, "path": a.path, "range_chunk_rows": a.chunk_rows or "default"}
                for name in variants:
                    out[name] = {"ms_best": round(min(times[name]), 3), "ms_all": [round(t, 3) for t in times[name]]}
                out["range_over_search"] = round(out["search_range"]["ms_best"] / out["search"]["ms_best"], 3)
                out["stats_of_one_call"] = stats
                out["same_bits_as_masked_search"] = same
                out["counts_equal_deep_search"] = counts_ok
                summary[f"m{m}_r{in_range}"] = [out["search_range"]["ms_best"], out["search"]["ms_best"]]
                print(json.dumps(out), flush=True)
    print(json.dumps({"summary_ms_best_range_vs_search": summary}))


if __name__ == "__main__":
    main()
