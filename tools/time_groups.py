"""Time `Mi355Index.search_groups` on one GPU next to the way a caller fused sub-query lists before it existed.

    python tools/time_groups.py --rows 1000000 --dim 768 --groups 256 --per-group 4 --k 10 --fetch-k 20 --repeats 5

Timed with the host clock around calls that are complete on return, after one warm-up of every variant; the variants alternate
inside every repeat, best and all values are kept:
  search         (a) search of the groups x per-group sub-queries at fetch_k, host buffers: the floor both ways share
  search_groups  (b) search_groups(Q, offsets, k, fetch_k), host buffers: (a) with the merge behind it on the device and
                 [G, k] instead of [S, fetch_k] downloaded
  host_merge     (c) the way available before: (a), then `merge_groups_host` (numpy, one pass per group)
Also checks that (b) and (c) return the same bits (values, rows, counts).  Prints one JSON line.
The corpus is Gaussian: one generated chunk, its columns rotated by the chunk number; the sub-queries of a group are noisy
copies of one vector, so their lists overlap as the lists of a decomposed question do."""

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
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--per-group", type=int, default=4)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch-k", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index
    from autorag_research_amd.sharded import merge_groups_host

    rng = np.random.default_rng(a.seed)
    n, d, G, per, k, f = a.rows, a.dim, a.groups, a.per_group, a.k, a.fetch_k
    S = G * per
    chunk = min(n, 250_000)
    base = rng.standard_normal((chunk, d), dtype=np.float32)
    centres = rng.standard_normal((G, d), dtype=np.float32)
    Q = (np.repeat(centres, per, axis=0) + 0.5 * rng.standard_normal((S, d), dtype=np.float32)).astype(np.float32)
    offs = (np.arange(G + 1) * per).astype(np.int32)

    with Mi355Index(d) as idx:
        for c, r0 in enumerate(range(0, n, chunk)):
            idx.add(np.roll(base, c, axis=1)[:min(chunk, n - r0)])

        def host_merge():
            dist, rows = idx.search(Q, f)
            return merge_groups_host(dist, rows, offs, k)

        variants = {"search": lambda: idx.search(Q, f), "search_groups": lambda: idx.search_groups(Q, offs, k, f),
                    "host_merge": host_merge}
        times = {name: [] for name in variants}
        last = {}
        for rep in range(a.repeats + 1):                          # (repeat 0: warm-up of every variant, not kept)
            for name, fn in variants.items():
                t0 = time.perf_counter()
                last[name] = fn()
                if rep:
                    times[name].append((time.perf_counter() - t0) * 1e3)
            print(f"repeat {rep} done", file=sys.stderr, flush=True)
        out = {"rows": n, "dim": d, "groups": G, "per_group": per, "subqueries": S, "k": k, "fetch_k": f, "repeats": a.repeats}
        for name in variants:
            out[name] = {"ms_best": round(min(times[name]), 3), "ms_all": [round(t, 3) for t in times[name]]}
        out["merge_ms_device"] = round(out["search_groups"]["ms_best"] - out["search"]["ms_best"], 3)
        out["merge_ms_host"] = round(out["host_merge"]["ms_best"] - out["search"]["ms_best"], 3)
        out["host_over_groups"] = round(out["host_merge"]["ms_best"] / out["search_groups"]["ms_best"], 2)
        (gv, gr, gc), (hv, hr, hc) = last["search_groups"], last["host_merge"]
        out["same_bits"] = bool(np.array_equal(gr, hr) and np.array_equal(gc, hc) and np.array_equal(np.isnan(gv), np.isnan(hv))
                                and np.array_equal(gv[~np.isnan(gv)].view(np.uint64), hv[~np.isnan(hv)].view(np.uint64)))
        out["mean_union"] = round(float(np.mean(gc)), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
