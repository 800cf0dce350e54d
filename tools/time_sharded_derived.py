"""Time the sharded range, by-row and MMR entry points on one GPU at world size 1, over the library's RCCL communicator, next to
their local entry points on the same index in the same run.

    python tools/time_sharded_derived.py --rows 1000000 --dim 768 --queries 1024 --repeats 5

A one-GPU box cannot show what sharding buys: at world 1 the sharded form does the local work plus the staging -- payload
buffers, one all-gather per block (per sub-block for the MMR stage), the fold, the merge.  The ratio sharded / local prices
that staging and is the baseline for the first multi-GPU run; no threshold is set on it.

Families (k = 10, fetch_k = 100, a radius per query that admits about 10 rows):
    range        search_range_device            / search_range_sharded_device
    rows         search_rows_device             / search_rows_sharded_device
    range_rows   search_range_rows_device       / search_range_rows_sharded_device
    mmr          search_mmr_device              / search_mmr_sharded_device
    mmr_select   mmr_select (host pools [B, 100]) / mmr_select_sharded
The two legs of a family alternate inside every repeat; the host clock runs around calls that are complete on return, after
one warm-up of each leg; best and all values are kept.  The two results must be equal bit for bit.  Stat "shard_gather_bytes"
is printed per sharded call.  One JSON line per family and one summary line.
The corpus is Gaussian: one generated chunk, its columns rotated by the chunk number."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def same_bits(a, b) -> bool:
    ok = True
    for x, y in zip(a, b):
        if x.dtype.kind == "f":
            nan = np.isnan(y)
            ok &= bool(np.array_equal(np.isnan(x), nan) and np.array_equal(x[~nan].view(np.uint64), y[~nan].view(np.uint64)))
        else:
            ok &= bool(np.array_equal(x, y))
    return ok


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch-k", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n, d, B, k, fk = a.rows, a.dim, a.queries, a.k, a.fetch_k
    chunk = min(n, 250_000)
    base = rng.standard_normal((chunk, d), dtype=np.float32)
    Q = rng.standard_normal((B, d), dtype=np.float32)
    ids = np.sort(rng.choice(n, size=B, replace=False)).astype(np.int64)
    summary = {}
    with Mi355Index(d) as idx:
        for c, r0 in enumerate(range(0, n, chunk)):
            idx.add(np.roll(base, c, axis=1)[:min(chunk, n - r0)])
        idx.comm_init(0, 1, Mi355Index.comm_unique_id())
        radius_q = idx.search(Q, k)[0][:, -1]                       # admits the k nearest rows of each query
        radius_r = idx.search_rows(ids, k)[0][:, -1]                # ... and of each stored row, itself left out
        pools = idx.search(Q, fk)[1]
        width = max(k, fk)
        q_dev = idx.dev_alloc(Q.nbytes)
        od, orr, oc = idx.dev_alloc(B * width * 8), idx.dev_alloc(B * width * 8), idx.dev_alloc(B * 8)
        try:
            idx.dev_upload(q_dev, Q)

            def download(with_count):
                gd, gr, gc = np.empty((B, k)), np.empty((B, k), dtype=np.int64), np.empty(B, dtype=np.int64)
                idx.dev_download(od, gd)
                idx.dev_download(orr, gr)
                if with_count:
                    idx.dev_download(oc, gc)
                return (gd, gr, gc) if with_count else (gd, gr)

            families = {
                "range": (True, lambda: idx.search_range_device(q_dev, B, radius_q, k, od, orr, oc),
                          lambda: idx.search_range_sharded_device(q_dev, B, radius_q, k, od, orr, oc)),
                "rows": (False, lambda: idx.search_rows_device(ids, k, od, orr),
                         lambda: idx.search_rows_sharded_device(ids, k, od, orr)),
                "range_rows": (True, lambda: idx.search_range_rows_device(ids, radius_r, k, od, orr, oc),
                               lambda: idx.search_range_rows_sharded_device(ids, radius_r, k, od, orr, oc)),
                "mmr": (False, lambda: idx.search_mmr_device(q_dev, B, k, fk, od, orr),
                        lambda: idx.search_mmr_sharded_device(q_dev, B, k, fk, od, orr)),
                "mmr_select": (None, lambda: idx.mmr_select(Q, k, pools), lambda: idx.mmr_select_sharded(Q, k, pools)),
            }
            for name, (with_count, local, sharded) in families.items():
                times = {"local": [], "sharded": []}
                results, gather = {}, 0
                for rep in range(a.repeats + 1):                    # (repeat 0: warm-up of both legs, not kept)
                    for leg, fn in (("local", local), ("sharded", sharded)):
                        before = idx.stat("shard_gather_bytes")
                        t0 = time.perf_counter()
                        got = fn()
                        if rep:
                            times[leg].append((time.perf_counter() - t0) * 1e3)
                        if leg == "sharded":
                            gather = idx.stat("shard_gather_bytes") - before
                        if rep == a.repeats:                        # (outside the clock: the device legs' results)
                            results[leg] = got if with_count is None else download(with_count)
                tl, ts = min(times["local"]), min(times["sharded"])
                out = {"family": name, "rows": n, "dim": d, "queries": B, "k": k, "fetch_k": fk, "repeats": a.repeats, "world": 1,
                       "local": {"ms_best": round(tl, 3), "ms_all": [round(t, 3) for t in times["local"]]},
                       "sharded": {"ms_best": round(ts, 3), "ms_all": [round(t, 3) for t in times["sharded"]]},
                       "sharded_over_local": round(ts / tl, 3), "shard_gather_bytes_per_call": int(gather),
                       "sharded_equals_local": same_bits(results["sharded"], results["local"])}
                if with_count:
                    out["mean_count"] = round(float(results["local"][2].mean()), 2)
                summary[name] = [out["local"]["ms_best"], out["sharded"]["ms_best"], out["sharded_over_local"]]
                print(json.dumps(out), flush=True)
        finally:
            for p in (q_dev, od, orr, oc):
                idx.dev_free(p)
    print(json.dumps({"summary_ms_best_local_sharded_ratio": summary}))


if __name__ == "__main__":
    main()
