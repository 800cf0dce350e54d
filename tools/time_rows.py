"""Time `Mi355Index.search_rows_device` on one GPU next to the ordinary search of the same vectors and next to the host flow
it replaces, in the same run on the same index.

    python tools/time_rows.py --rows 1000000 --dim 768 --queries 1024 --repeats 5 [--no-graph]

B row ids are drawn at random.  For k = 10 and k = 32 these legs alternate inside every repeat:
    (a) `search_device` at k + 1 on the same vectors, already gathered into a device buffer -- and (a0) the same at k, which
        shows what the inner pass's k + 1 costs where it crosses into the next k class of the search (k = 32);
    (b) `search_rows_device` at k;
    (c) the host flow: `get_rows` per id, `search` at k + 1, a numpy strip of each row's own id.
Timed with the host clock around calls that are complete on return, after one warm-up of every leg; best and all values are
kept.  (b) - (a) is printed next to the spread between the repeats of (a).  The three results are compared: (a) stripped on
the host and (c) must equal (b) bit for bit (the corpus has no exact duplicates, so the host strip is safe here).
    (d) `knn_graph(10)` over all rows, wall time, once.
Prints one JSON line per k, one for the graph and one summary line.
The corpus is Gaussian: one generated chunk, its columns rotated by the chunk number."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def strip_self(dist, rows, ids, k):
    """the host's version of the drop: the row's own id out of a top-(k + 1) list, else the list cut to k"""
    own = rows == ids[:, None]
    pos = np.where(own.any(axis=1), own.argmax(axis=1), k)
    take = np.arange(k)[None, :] + (np.arange(k)[None, :] >= pos[:, None])
    return np.take_along_axis(dist, take, axis=1), np.take_along_axis(rows, take, axis=1)


def same_bits(a, b) -> bool:
    (ad, ar), (bd, br) = a, b
    nan = np.isnan(bd)
    return bool(np.array_equal(ar, br) and np.array_equal(np.isnan(ad), nan)
                and np.array_equal(ad[~nan].view(np.uint64), bd[~nan].view(np.uint64)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--path", default="auto")
    ap.add_argument("--no-graph", action="store_true", help="skip leg (d), the k-NN graph of the whole corpus")
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n, d, B = a.rows, a.dim, a.queries
    chunk = min(n, 250_000)
    base = rng.standard_normal((chunk, d), dtype=np.float32)
    ids = np.sort(rng.choice(n, size=B, replace=False)).astype(np.int64)
    summary = {}
    with Mi355Index(d) as idx:
        for c, r0 in enumerate(range(0, n, chunk)):
            idx.add(np.roll(base, c, axis=1)[:min(chunk, n - r0)])
        idx.set_option("path", a.path)
        V = np.concatenate([idx.get_rows(int(r), 1) for r in ids])
        kmax = 33
        q_dev, od, orr = idx.dev_alloc(V.nbytes), idx.dev_alloc(B * kmax * 8), idx.dev_alloc(B * kmax * 8)
        try:
            idx.dev_upload(q_dev, V)
            for k in (10, 32):
                def download(width):
                    gd, gr = np.empty((B, width)), np.empty((B, width), dtype=np.int64)
                    idx.dev_download(od, gd)
                    idx.dev_download(orr, gr)
                    return gd, gr

                def host_flow():
                    vecs = np.concatenate([idx.get_rows(int(r), 1) for r in ids])
                    return strip_self(*idx.search(vecs, k + 1), ids, k)

                legs = {"a0_search_device_k": lambda: idx.search_device(q_dev, B, k, od, orr),
                        "a_search_device_k_plus_1": lambda: idx.search_device(q_dev, B, k + 1, od, orr),
                        "b_search_rows_device": lambda: idx.search_rows_device(ids, k, od, orr),
                        "c_host_flow": host_flow}
                times = {name: [] for name in legs}
                results = {}
                for rep in range(a.repeats + 1):                  # (repeat 0: warm-up of every leg, not kept)
                    for name, fn in legs.items():
                        t0 = time.perf_counter()
                        got = fn()
                        if rep:
                            times[name].append((time.perf_counter() - t0) * 1e3)
                        if rep == a.repeats:                      # (outside the clock: the device legs' results)
                            results[name] = got if name == "c_host_flow" else download(k + 1 if name.startswith("a_") else k)
                ta, tb = times["a_search_device_k_plus_1"], times["b_search_rows_device"]
                out = {"rows": n, "dim": d, "queries": B, "k": k, "repeats": a.repeats, "path": a.path}
                for name in legs:
                    out[name] = {"ms_best": round(min(times[name]), 3), "ms_all": [round(t, 3) for t in times[name]]}
                out["b_minus_a_ms"] = round(min(tb) - min(ta), 3)
                out["spread_of_a_ms"] = round(max(ta) - min(ta), 3)
                out["b_minus_a_within_spread_of_a"] = bool(abs(min(tb) - min(ta)) <= max(ta) - min(ta))
                out["k_plus_1_minus_k_ms"] = round(min(ta) - min(times["a0_search_device_k"]), 3)   # (k = 32: the next k class)
                out["host_flow_over_b"] = round(min(times["c_host_flow"]) / min(tb), 1)
                b_res = results["b_search_rows_device"]
                out["a_stripped_equals_b"] = same_bits(strip_self(*results["a_search_device_k_plus_1"], ids, k), b_res)
                out["c_equals_b"] = same_bits(results["c_host_flow"], b_res)
                summary[f"k{k}"] = [out[name]["ms_best"] for name in legs]
                print(json.dumps(out), flush=True)
        finally:
            for p in (q_dev, od, orr):
                idx.dev_free(p)
        if not a.no_graph:
            t0 = time.perf_counter()
            gd, gr = idx.knn_graph(10)
            wall = time.perf_counter() - t0
            check = same_bits((gd[ids], gr[ids]), idx.search_rows(ids, 10))
            out = {"rows": n, "dim": d, "knn_graph_k": 10, "block": 1024, "wall_s": round(wall, 3),
                   "ms_per_block_of_1024": round(wall * 1e3 / ((n + 1023) // 1024), 3), "sample_equals_search_rows": check,
                   "rows_with_all_k_neighbours": int((gr[:, -1] >= 0).sum())}
            summary["knn_graph_10_wall_s"] = out["wall_s"]
            print(json.dumps(out), flush=True)
    print(json.dumps({"summary_ms_best_a0_a_b_c": summary}))


if __name__ == "__main__":
    main()
