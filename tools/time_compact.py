"""Time `Mi355Index.compact()` on one GPU next to the rebuild it replaces (a new index + `add_device` of rows already in HBM).

    python tools/time_compact.py --rows 10000000 --dim 768 --repeats 3

Timed with the host clock around calls that are complete on return, best of `--repeats`:
  head    compact() after removing the first 10 % of the rows (the dead head)
  random  compact() after removing 10 % of the rows at random
  one     compact() after removing one row of the first group (everything behind it moves)
  rebuild a new index + add_device of all rows from a device buffer
  pass    one search of 1024 queries, k = 10, before and after the compaction, with the retry / fallback counts of that pass
Prints one JSON line.  The corpus is Gaussian: one generated chunk, its columns rotated by the chunk number (distinct rows
without generating every value)."""

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
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n, d = a.rows, a.dim
    chunk = min(n, 1_000_000)
    base = rng.standard_normal((chunk, d), dtype=np.float32)
    Q = rng.standard_normal((a.queries, d), dtype=np.float32)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    with Mi355Index(8) as owner:                                   # (owns the device buffer the rebuilds read)
        src = owner.dev_alloc(n * d * 4)
        for c, r0 in enumerate(range(0, n, chunk)):
            m = min(chunk, n - r0)
            owner.dev_upload(src + r0 * d * 4, np.roll(base, c, axis=1)[:m])

        def build() -> Mi355Index:
            idx = Mi355Index(d)
            idx.add_device(src, n)
            idx.synchronize()
            return idx

        def search_pass(idx) -> dict:
            idx.search(Q, 10)                                      # (warm-up: per-search state, code objects)
            best, stats = None, {}
            for _ in range(a.repeats):
                idx.reset_stats()
                t = timed(lambda: idx.search(Q, 10))
                if best is None or t < best:
                    best = t
                    stats = {key: idx.stat(key) for key in ("retry_queries", "fallback_queries", "passes", "screen_rows")}
            return {"ms": round(best, 3), **stats}

        build().close()                                            # warm-up (code objects, allocator)
        rebuild = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            idx = build()
            rebuild.append((time.perf_counter() - t0) * 1e3)
            idx.close()
        scenarios = {"head": np.arange(n // 10), "random": np.sort(rng.choice(n, n // 10, replace=False)),
                     "one": np.array([min(7, n - 1)])}
        out = {"rows": n, "dim": d, "repeats": a.repeats, "queries": a.queries,
               "rebuild_device_ms": {"best": round(min(rebuild), 3), "all": [round(t, 3) for t in rebuild]}}
        for name, removed in scenarios.items():
            times, res = [], {}
            for rep in range(a.repeats):
                idx = build()
                try:
                    idx.remove_rows(removed)
                    if rep == 0:
                        res["pass_before"] = search_pass(idx)
                    idx.reset_stats()
                    times.append(timed(idx.compact))
                    if rep == 0:
                        res["moved_rows"] = idx.stat("compact_moved_rows")
                        res["size_after"] = len(idx)
                        res["pass_after"] = search_pass(idx)
                finally:
                    idx.close()
            res["compact_ms"] = {"best": round(min(times), 3), "all": [round(t, 3) for t in times]}
            out[name] = res
        owner.dev_free(src)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
