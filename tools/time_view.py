"""Time `Mi355Index.view` on one GPU next to `search_subset_device` over the same lists.

    python tools/time_view.py --rows 1000000 --dim 768 --queries 1024 --k 10 --repeats 5

Per list (m = 10 000 and 100 000 rows drawn at random, and every row):
  build_ms     `idx.view(row_ids)`: list hygiene, the gather, the view's own add paths -- complete on return
  view_ms      one block of queries through `view.search_device` (the ordinary AUTO path: screens, prunes, exact re-score)
  subset_ms    the same block through `idx.search_subset_device` on the parent (the exact scan walking the list)
  break_even   the number of query blocks from which build + blocks on the view cost less than the same blocks through
               search_subset: ceil(build_ms / (subset_ms - view_ms)); "never" when a block on the view is no faster
Timed with the host clock around calls that are complete on return (queries and outputs stay in device memory), after one
warm-up of every shape; the variants alternate inside every repeat; best and all values are kept.  The view's answer is
compared with search_subset's (ids and distance bits).  Prints a table and one JSON line.
The corpus is Gaussian: one generated chunk, its columns rotated by the chunk number."""

from __future__ import annotations

import argparse
import json
import math
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

    def ms(fn) -> float:
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    with Mi355Index(d) as idx:
        for c, r0 in enumerate(range(0, n, chunk)):
            idx.add(np.roll(base, c, axis=1)[:min(chunk, n - r0)])
        pq, od, orr = idx.dev_alloc(Q.nbytes), idx.dev_alloc(B * k * 8), idx.dev_alloc(B * k * 8)
        idx.dev_upload(pq, Q)

        def download():
            gd, gr = np.empty((B, k)), np.empty((B, k), dtype=np.int64)
            idx.dev_download(od, gd)
            idx.dev_download(orr, gr)
            return gd.view(np.uint64).copy(), gr

        out = {"rows": n, "dim": d, "queries": B, "k": k, "repeats": a.repeats, "lists": {}}
        for m, ids in lists.items():
            t = {"build": [], "view": [], "subset": [], "full": []}
            for rep in range(a.repeats + 1):                      # (repeat 0: warm-up of every shape, not kept)
                holder = []
                tb = ms(lambda: holder.append(idx.view(row_ids=ids)))
                v = holder[0]
                tv = ms(lambda: v.search_device(pq, B, k, od, orr))
                got = download()
                ts = ms(lambda: idx.search_subset_device(pq, B, k, ids, od, orr))
                want = download()
                tf = ms(lambda: idx.search_device(pq, B, k, od, orr))
                agree = np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                screens = v.stat("screen_launches")
                resident = v.stat("hbm_bytes_resident")
                v.close()
                if rep:
                    for key, val in zip(("build", "view", "subset", "full"), (tb, tv, ts, tf)):
                        t[key].append(val)
            best = {key: min(val) for key, val in t.items()}
            gain = best["subset"] - best["view"]
            out["lists"][str(m)] = {
                "m": m, "build_ms": round(best["build"], 3), "view_ms": round(best["view"], 3),
                "subset_ms": round(best["subset"], 3), "unrestricted_ms": round(best["full"], 3),
                "break_even_blocks": math.ceil(best["build"] / gain) if gain > 0 else None,
                "build_ms_all": [round(x, 3) for x in t["build"]], "view_ms_all": [round(x, 3) for x in t["view"]],
                "subset_ms_all": [round(x, 3) for x in t["subset"]], "view_screen_launches": screens,
                "view_hbm_bytes": resident, "results_agree": bool(agree)}
        for p in (pq, od, orr):
            idx.dev_free(p)
    print(f"# N = {n}, d = {d}, {B} queries per block, k = {k}; best of {a.repeats}, ms")
    print(f"# {'rows listed':>12} {'build':>9} {'view/block':>11} {'subset/block':>13} {'break-even blocks':>18}  agree")
    for r in out["lists"].values():
        be = "never" if r["break_even_blocks"] is None else str(r["break_even_blocks"])
        print(f"# {r['m']:>12} {r['build_ms']:>9.3f} {r['view_ms']:>11.3f} {r['subset_ms']:>13.3f} {be:>18}  {r['results_agree']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
