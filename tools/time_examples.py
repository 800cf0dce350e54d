"""Time `Mi355Index.search_examples_device` and `search_feedback_device` on one GPU next to the ordinary searches they wrap
and next to the host flows they replace, in the same run on the same index.

    python tools/time_examples.py --rows 1000000 --dim 768 --queries 1024 --repeats 5

B Gaussian queries; for the search by examples every slot lists mp random rows as positives (mp = 8 and 64), the query as
base.  These legs alternate inside every repeat:
    (a)  `search_device` of the queries at k -- the floor;
    (a+) `search_device` of the COMBINED vectors at k + mp, the depth of (b)'s inner pass: what that depth costs by itself
         (it may be served by the next k class of the search: <= 32 | 33 ... 128 | above);
    (b)  `search_examples_device` at k;
    (c)  the host flow: `get_rows` per id, the normalised mean in numpy, `search` at k + mp, a numpy strike of the listed ids.
For the feedback (fb_k = 10 and 100):
    (d0) the two `search_device` calls it wraps: the queries at fb_k, the moved queries at k;
    (d)  `search_feedback_device`;
    (e)  the host flow: `search` at fb_k, `get_rows` per id, numpy, `search` at k.
Timed with the host clock around calls that are complete on return, after one warm-up of every leg; best and all values are
kept.  (b) - (a+) and (d) - (d0) are printed next to the spread between the repeats of (a).  Results are compared in the same
run: (a+) struck on the host and (d0) must equal (b) and (d) bit for bit; the host flows form their mean in numpy's order,
not the library's, so they are compared by the share of equal rows.
Prints one JSON line per setting and one summary line.  The corpus is Gaussian: one generated chunk, its columns rotated by
the chunk number."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def strike(dist, rows, listed, k):
    """the host's version of the strike: the listed ids out of a deeper list, the first k survivors"""
    od = np.full((len(rows), k), np.nan)
    orr = np.full((len(rows), k), -1, dtype=np.int64)
    keep = ~(rows[:, :, None] == listed[:, None, :]).any(axis=2)
    for b in range(len(rows)):
        at = np.flatnonzero(keep[b])[:k]
        od[b, :len(at)], orr[b, :len(at)] = dist[b, at], rows[b, at]
    return od, orr


def same_bits(a, b) -> bool:
    (ad, ar), (bd, br) = a, b
    nan = np.isnan(bd)
    return bool(np.array_equal(ar, br) and np.array_equal(np.isnan(ad), nan)
                and np.array_equal(ad[~nan].view(np.uint64), bd[~nan].view(np.uint64)))


def unit_mean(idx, ids):
    """[B, m] ids -> the mean of the rows' unit vectors, float64, one `get_rows` per id"""
    out = []
    for line in ids:
        v = np.concatenate([idx.get_rows(int(r), 1) for r in line]).astype(np.float64)
        out.append((v / np.linalg.norm(v, axis=1, keepdims=True)).mean(axis=0))
    return np.stack(out)


def run_legs(legs, repeats, fetch):
    """every leg once per repeat, in turn; repeat 0 warms up.  -> (times [ms] per leg, the last repeat's results)"""
    times = {name: [] for name in legs}
    results = {}
    for rep in range(repeats + 1):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            got = fn()
            if rep:
                times[name].append((time.perf_counter() - t0) * 1e3)
            if rep == repeats:                              # (outside the clock: the device legs' results)
                results[name] = fetch(name, got)
    return times, results


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--path", default="auto")
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n, d, B, k = a.rows, a.dim, a.queries, a.k
    chunk = min(n, 250_000)
    base = rng.standard_normal((chunk, d), dtype=np.float32)
    Q = rng.standard_normal((B, d), dtype=np.float32)
    summary = {}
    with Mi355Index(d) as idx:
        for c, r0 in enumerate(range(0, n, chunk)):
            idx.add(np.roll(base, c, axis=1)[:min(chunk, n - r0)])
        idx.set_option("path", a.path)
        wmax = 128
        q_dev, q2_dev = idx.dev_alloc(Q.nbytes), idx.dev_alloc(Q.nbytes)
        ok_dev, od, orr = idx.dev_alloc(4 * B), idx.dev_alloc(B * wmax * 8), idx.dev_alloc(B * wmax * 8)

        def download(width):
            gd, gr = np.empty((B, width)), np.empty((B, width), dtype=np.int64)
            idx.dev_download(od, gd)
            idx.dev_download(orr, gr)
            return gd, gr

        def line(times, legs):
            return {name: {"ms_best": round(min(times[name]), 3), "ms_all": [round(t, 3) for t in times[name]]} for name in legs}

        try:
            idx.dev_upload(q_dev, Q)
            for mp in (8, 64):
                pos = rng.integers(0, n, size=(B, mp)).astype(np.int64)
                idx.combine_rows_device(pos, None, q_dev, q2_dev, ok_dev)       # the combined vectors, for leg (a+)

                def host_flow():
                    qn = Q.astype(np.float64) / np.linalg.norm(Q.astype(np.float64), axis=1, keepdims=True)
                    moved = (qn + unit_mean(idx, pos)).astype(np.float32)
                    return strike(*idx.search(moved, k + mp), pos, k)

                legs = {"a_search_device_k": lambda: idx.search_device(q_dev, B, k, od, orr),
                        "a_plus_search_device_k_plus_mp": lambda: idx.search_device(q2_dev, B, k + mp, od, orr),
                        "b_search_examples_device": lambda: idx.search_examples_device(pos, None, q_dev, k, od, orr),
                        "c_host_flow": host_flow}
                widths = {"a_search_device_k": k, "a_plus_search_device_k_plus_mp": k + mp, "b_search_examples_device": k}
                times, res = run_legs(legs, a.repeats, lambda name, got: got if name == "c_host_flow" else download(widths[name]))
                ta, tp, tb = (times[x] for x in ("a_search_device_k", "a_plus_search_device_k_plus_mp", "b_search_examples_device"))
                out = {"rows": n, "dim": d, "queries": B, "k": k, "mp": mp, "repeats": a.repeats, "path": a.path, **line(times, legs)}
                out["b_minus_a_ms"] = round(min(tb) - min(ta), 3)
                out["b_minus_a_plus_ms"] = round(min(tb) - min(tp), 3)
                out["depth_cost_a_plus_minus_a_ms"] = round(min(tp) - min(ta), 3)
                out["spread_of_a_ms"] = round(max(ta) - min(ta), 3)
                out["b_minus_a_plus_within_spread_of_a"] = bool(abs(min(tb) - min(tp)) <= max(ta) - min(ta))
                out["host_flow_over_b"] = round(min(times["c_host_flow"]) / min(tb), 1)
                b_res = res["b_search_examples_device"]
                out["a_plus_struck_equals_b"] = same_bits(strike(*res["a_plus_search_device_k_plus_mp"], pos, k), b_res)
                out["c_rows_equal_share"] = round(float((res["c_host_flow"][1] == b_res[1]).mean()), 4)
                summary[f"examples_mp{mp}"] = [out[name]["ms_best"] for name in legs]
                print(json.dumps(out), flush=True)
            for fb_k in (10, 100):
                d1, r1 = idx.search(Q, fb_k)
                idx.combine_rows_device(r1, None, q_dev, q2_dev, ok_dev, 1.0, 0.75)   # the moved queries, for leg (d0)

                def two_searches():
                    idx.search_device(q_dev, B, fb_k, od, orr)
                    idx.search_device(q2_dev, B, k, od, orr)

                def host_flow():
                    _, rows1 = idx.search(Q, fb_k)
                    qn = Q.astype(np.float64) / np.linalg.norm(Q.astype(np.float64), axis=1, keepdims=True)
                    return idx.search((qn + 0.75 * unit_mean(idx, rows1)).astype(np.float32), k)

                legs = {"a_search_device_k": lambda: idx.search_device(q_dev, B, k, od, orr),
                        "d0_two_search_device": two_searches,
                        "d_search_feedback_device": lambda: idx.search_feedback_device(q_dev, B, k, fb_k, od, orr),
                        "e_host_flow": host_flow}
                times, res = run_legs(legs, a.repeats, lambda name, got: got if name == "e_host_flow" else download(k))
                ta, t0_, td = (times[x] for x in ("a_search_device_k", "d0_two_search_device", "d_search_feedback_device"))
                out = {"rows": n, "dim": d, "queries": B, "k": k, "fb_k": fb_k, "repeats": a.repeats, "path": a.path, **line(times, legs)}
                out["d_minus_d0_ms"] = round(min(td) - min(t0_), 3)
                out["spread_of_a_ms"] = round(max(ta) - min(ta), 3)
                out["d_minus_d0_within_spread_of_a"] = bool(abs(min(td) - min(t0_)) <= max(ta) - min(ta))
                out["host_flow_over_d"] = round(min(times["e_host_flow"]) / min(td), 1)
                d_res = res["d_search_feedback_device"]
                out["d0_equals_d"] = same_bits(res["d0_two_search_device"], d_res)
                out["e_rows_equal_share"] = round(float((res["e_host_flow"][1] == d_res[1]).mean()), 4)
                out["lists_moved_by_feedback"] = int((d_res[1] != idx.search(Q, k)[1]).any(axis=1).sum())
                summary[f"feedback_fb{fb_k}"] = [out[name]["ms_best"] for name in legs]
                print(json.dumps(out), flush=True)
        finally:
            for p in (q_dev, q2_dev, ok_dev, od, orr):
                idx.dev_free(p)
    print(json.dumps({"summary_ms_best_per_leg": summary}))


if __name__ == "__main__":
    main()
