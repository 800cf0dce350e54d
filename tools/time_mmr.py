"""Time `Mi355Index.search_mmr_device` on one GPU next to the search it starts with and the recipe it replaces.

    python tools/time_mmr.py --rows 1000000 --dim 768 --queries 1024 --k 10 --fetch-k 50 100 200 --repeats 5

Timed with the host clock around calls that are complete on return, after one warm-up of every shape; the variants alternate
inside every repeat, best and all values are kept.  Per fetch_k:
  search      (a) search_device at k = fetch_k, device buffers: the floor -- (b) minus (a) is what the selection costs
  search_mmr  (b) search_mmr_device at (k, fetch_k, lambda), device buffers
  host_recipe (c) what a caller does without it: search at fetch_k (host buffers), gather C[rows] from a HOST copy of the
              corpus, MMR in numpy (all queries at once: normalised candidates, one batched matmul per pick).  fp32 BLAS sums, not
              the library's chains: timed only, not compared
Also checks that (b) at lambda = 1 returns the bits of search_device at k.  Prints one JSON line.
The corpus is Gaussian: one generated chunk, its columns rotated by the chunk number."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def numpy_mmr(dist: np.ndarray, cand: np.ndarray, k: int, lam: float) -> np.ndarray:
    """positions picked, [B, k]: cosine MMR over cand [B, f, d] with query similarities 1 - dist [B, f]"""
    B, f, _ = cand.shape
    cand = cand / np.linalg.norm(cand, axis=2, keepdims=True)
    sq = 1.0 - dist
    ms = np.full((B, f), -np.inf)
    taken = np.zeros((B, f), dtype=bool)
    picks = np.zeros((B, k), dtype=np.int64)
    rows = np.arange(B)
    cur = np.zeros(B, dtype=np.int64)
    for t in range(k):
        if t:
            cur = np.where(taken, -np.inf, lam * sq - (1.0 - lam) * ms).argmax(axis=1)
        picks[:, t] = cur
        taken[rows, cur] = True
        if t + 1 < k:
            ms = np.maximum(ms, np.matmul(cand, cand[rows, cur][:, :, None])[:, :, 0])
    return picks


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch-k", type=int, nargs="+", default=[50, 100, 200])
    ap.add_argument("--lambda-mult", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n, d, B, k, lam = a.rows, a.dim, a.queries, a.k, a.lambda_mult
    chunk = min(n, 250_000)
    base = rng.standard_normal((chunk, d), dtype=np.float32)
    Q = rng.standard_normal((B, d), dtype=np.float32)
    C = np.empty((n, d), dtype=np.float32)             # (c)'s host copy of the corpus

    with Mi355Index(d) as idx:
        for c, r0 in enumerate(range(0, n, chunk)):
            C[r0:r0 + chunk] = np.roll(base, c, axis=1)[:min(chunk, n - r0)]
            idx.add(C[r0:r0 + chunk])
        fmax = max(a.fetch_k)
        pq, od, orr = idx.dev_alloc(Q.nbytes), idx.dev_alloc(B * fmax * 8), idx.dev_alloc(B * fmax * 8)
        idx.dev_upload(pq, Q)

        def host_recipe(f: int):
            dist, rows = idx.search(Q, f)
            pos = numpy_mmr(dist, C[rows], k, lam)
            return np.take_along_axis(rows, pos, axis=1)

        variants = {}
        for f in a.fetch_k:
            variants[f"search_{f}"] = lambda f=f: idx.search_device(pq, B, f, od, orr)
            variants[f"search_mmr_{f}"] = lambda f=f: idx.search_mmr_device(pq, B, k, f, od, orr, lam)
            variants[f"host_recipe_{f}"] = lambda f=f: host_recipe(f)
        times = {name: [] for name in variants}
        for rep in range(a.repeats + 1):                          # (repeat 0: warm-up of every shape, not kept)
            for name, fn in variants.items():
                t0 = time.perf_counter()
                fn()
                if rep:
                    times[name].append((time.perf_counter() - t0) * 1e3)
            print(f"repeat {rep} done", file=sys.stderr, flush=True)
        out = {"rows": n, "dim": d, "queries": B, "k": k, "lambda": lam, "repeats": a.repeats}
        for name in variants:
            out[name] = {"ms_best": round(min(times[name]), 3), "ms_all": [round(t, 3) for t in times[name]]}
        for f in a.fetch_k:
            idx.reset_stats()
            variants[f"search_mmr_{f}"]()
            out[f"selection_ms_{f}"] = round(out[f"search_mmr_{f}"]["ms_best"] - out[f"search_{f}"]["ms_best"], 3)
            out[f"recipe_over_mmr_{f}"] = round(out[f"host_recipe_{f}"]["ms_best"] / out[f"search_mmr_{f}"]["ms_best"], 2)
            out[f"mmr_pairs_scored_{f}"] = idx.stat("mmr_pairs_scored")
        # lambda = 1 is the ordinary top-k, bit for bit
        res = []
        for fn in (lambda: idx.search_device(pq, B, k, od, orr), lambda: idx.search_mmr_device(pq, B, k, fmax, od, orr, 1.0)):
            fn()
            gd, gr = np.empty((B, k)), np.empty((B, k), dtype=np.int64)
            idx.dev_download(od, gd)
            idx.dev_download(orr, gr)
            res.append((gd.view(np.uint64).copy(), gr))
        out["lambda_one_equals_search"] = bool(np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]))
        for p in (pq, od, orr):
            idx.dev_free(p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
