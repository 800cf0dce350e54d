"""Time `Mi355Index.search_maxsim_subset` on one GPU next to the other ways of searching MaxSim inside one list of documents.

    python tools/time_maxsim_subset.py --docs 1000000 --queries 16 --nq 32 --k 10 --repeats 5

The store is synthetic and built on the device (bench_support.run_maxsim's recipe: unit-norm Gaussian token vectors, d = 128,
U{60..180} vectors per document); a call is 16 queries x 32 vectors, k = 10.  Per list (m = 1 000, 10 000 and 100 000 documents
drawn at random, and every document), one call each of
  screen_ms   search_maxsim_subset with option maxsim_subset_screen = 1 (the list form of the bf16 screen)
  exact_ms    search_maxsim_subset with maxsim_subset_screen = 0 (the exact kernel over the list, device top-k)
  default_ms  search_maxsim_subset with the option at its default (-1)
  recipe_ms   what the retrieval service did before: maxsim_subset on the list tiled B times + np.lexsort on the host
  view_ms     view(doc_ids=list) build + search_maxsim on it + close (lists up to --view-max documents: a view of every
              document is a second copy of the store)
  full_ms     (the list of every document only) plain search_maxsim
Timed with the host clock around calls that are complete on return, after one warm-up of every shape; the variants alternate
inside every repeat; best and all values are kept.  The ids and fp32 distance bits of all variants of a list are compared in
the same run.  Prints a table and one JSON line; run the command twice and keep both outputs."""

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
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--nq", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--view-max", type=int, default=100_000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import torch

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n, d, B, nq, k = a.docs, 128, a.queries, a.nq, a.k
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed)
    lens = rng.integers(60, 181, size=n)
    qtok = rng.standard_normal((B * nq, d), dtype=np.float32)
    qtok /= np.linalg.norm(qtok, axis=1, keepdims=True)
    qoff = (np.arange(B + 1) * nq).astype(np.int32)
    lists = {m: rng.choice(n, m, replace=False).astype(np.int64) for m in (1_000, 10_000, 100_000) if m < n}
    lists[n] = np.arange(n, dtype=np.int64)

    def ms(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def bits(res):
        dist, rows = res
        return np.ascontiguousarray(dist, np.float32).view(np.uint32).copy(), np.asarray(rows, np.int64)

    with Mi355Index(d, device=0) as idx:
        per_chunk = 1 << 15
        for d0 in range(0, n, per_chunk):
            ln = lens[d0:d0 + per_chunk]
            x = torch.randn((int(ln.sum()), d), generator=g, device=dev, dtype=torch.float32)
            x /= x.norm(dim=1, keepdim=True)
            torch.cuda.synchronize()
            idx.add_multivec_device(x.data_ptr(), np.concatenate([[0], np.cumsum(ln)]).astype(np.int64))
            del x
        torch.cuda.empty_cache()

        def subset(screen, ids):
            idx.set_option("maxsim_subset_screen", screen)
            try:
                return idx.search_maxsim_subset(qtok, qoff, k, ids)
            finally:
                idx.set_option("maxsim_subset_screen", -1)

        def recipe(ids):   # Mi355RetrievalService._maxsim_within before search_maxsim_subset existed
            docs = np.sort(ids)
            scored = np.asarray(idx.maxsim_subset(qtok, qoff, np.tile(docs, (B, 1))), dtype=np.float32)
            dist, rows = np.full((B, k), np.nan, np.float32), np.full((B, k), -1, np.int64)
            for b in range(B):
                live = np.nonzero(~np.isnan(scored[b]))[0]
                best = live[np.lexsort((docs[live], scored[b, live]))[:k]]
                dist[b, :best.size], rows[b, :best.size] = scored[b, best], docs[best]
            return dist, rows

        def through_view(ids):
            with idx.view(doc_ids=ids) as v:
                return v.search_maxsim(qtok, qoff, k)

        out = {"docs": n, "dim": d, "queries": B, "nq": nq, "k": k, "repeats": a.repeats, "lists": {}}
        for m, ids in lists.items():
            variants = {"screen": lambda: subset(1, ids), "exact": lambda: subset(0, ids), "default": lambda: subset(-1, ids),
                        "recipe": lambda: recipe(ids)}
            if m <= a.view_max:
                variants["view"] = lambda: through_view(ids)
            if m == n:
                variants["full"] = lambda: idx.search_maxsim(qtok, qoff, k)
            t = {key: [] for key in variants}
            agree = True
            for rep in range(a.repeats + 1):                      # (repeat 0: warm-up of every shape, not kept)
                idx.reset_stats()
                got = {}
                for key, fn in variants.items():
                    el, res = ms(fn)
                    got[key] = bits(res)
                    if rep:
                        t[key].append(el)
                ref = got["exact"]
                agree = agree and all(np.array_equal(v[0], ref[0]) and np.array_equal(v[1], ref[1]) for v in got.values())
                stats = {s: idx.stat("maxsim_subset_" + s) for s in ("screened", "exact", "fallbacks")}
            out["lists"][str(m)] = {"m": m, **{key + "_ms": round(min(v), 3) for key, v in t.items()},
                                    **{key + "_ms_all": [round(x, 3) for x in v] for key, v in t.items()},
                                    "queries_by_path_last_repeat": stats, "results_agree": bool(agree)}
    cols = ("screen", "exact", "default", "recipe", "view", "full")
    print(f"# {n} documents of 60..180 vectors, d = {d}; {B} queries x {nq} vectors, k = {k}; best of {a.repeats}, ms per call")
    print("# " + f"{'docs listed':>12} " + " ".join(f"{c:>10}" for c in cols) + "  agree")
    for r in out["lists"].values():
        cells = " ".join(f"{r[c + '_ms']:>10.3f}" if c + "_ms" in r else f"{'-':>10}" for c in cols)
        print(f"# {r['m']:>12} {cells}  {r['results_agree']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
