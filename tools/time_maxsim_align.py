"""Time `Mi355Index.maxsim_align` / `maxsim_map` on one GPU next to `maxsim_subset` of the same arguments (the same MFMA work
without the argmax and without the per-vector outputs) and next to numpy over a host copy of just those candidates.

    python tools/time_maxsim_align.py --repeats 5

Two synthetic stores, unit-norm Gaussian token vectors, d = 128:
  colbert  --docs documents of U{60..140} vectors (about 100); a query is 32 vectors against 100 candidates drawn at random,
           B = 1 and B = 64 queries per call
  colpali  --pages pages of 1030 vectors; 24 query vectors against 10 pages, and the similarity map of one page
Per shape one call each of
  align_ms   maxsim_align (values, tokens and distances)
  subset_ms  maxsim_subset (distances only)
  numpy_ms   fp32 `q @ doc.T`, max and argmax per candidate over a host copy of the candidates (not the exact chain: a yardstick
             for "fetch the vectors and do it on the host", without the fetch)
  map_ms / map_numpy_ms   (colpali) maxsim_map of one (query, page) pair / `q @ page.T`
Timed with the host clock around calls that are complete on return, after one warm-up of every shape; the variants alternate
inside every repeat; best and all values are kept.  The distances of align and subset are compared bit for bit in the same run.
Prints a table and one JSON line."""

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
    ap.add_argument("--docs", type=int, default=4096)
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    d = 128

    def unit(n):
        v = rng.standard_normal((n, d), dtype=np.float32)
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def ms(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def measure(variants, agree):
        t = {key: [] for key in variants}
        ok = True
        for rep in range(a.repeats + 1):                      # (repeat 0: warm-up of every shape, not kept)
            got = {}
            for key, fn in variants.items():
                el, got[key] = ms(fn)
                if rep:
                    t[key].append(el)
            ok = ok and agree(got)
        return {**{key + "_ms": round(min(v), 3) for key, v in t.items()},
                **{key + "_ms_all": [round(x, 3) for x in v] for key, v in t.items()}, "results_agree": bool(ok)}

    def numpy_align(q, qoff, ids, docs):
        out = []
        for b in range(ids.shape[0]):
            qb = q[qoff[b]:qoff[b + 1]]
            for i in ids[b]:
                s = qb @ docs[int(i)].T
                out.append((s.max(axis=1), s.argmax(axis=1)))
        return out

    def same_dist(got):
        x, y = got["align"].dist, got["subset"]
        return np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))

    out = {"dim": d, "repeats": a.repeats, "shapes": {}}
    lens = rng.integers(60, 141, size=a.docs)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tok = unit(int(off[-1]))
    docs = [tok[off[i]:off[i + 1]] for i in range(a.docs)]
    with Mi355Index(d, device=0) as idx:
        idx.add_multivec(tok, off)
        for B in (1, 64):
            q, qoff = unit(B * 32), (np.arange(B + 1) * 32).astype(np.int32)
            ids = np.stack([rng.choice(a.docs, 100, replace=False) for _ in range(B)]).astype(np.int64)
            out["shapes"][f"colbert_B{B}"] = measure(
                {"align": lambda: idx.maxsim_align(q, qoff, ids), "subset": lambda: idx.maxsim_subset(q, qoff, ids),
                 "numpy": lambda: numpy_align(q, qoff, ids, docs)}, same_dist)
    pages = [unit(1030) for _ in range(a.pages)]
    with Mi355Index(d, device=0) as idx:
        idx.add_multivec(np.concatenate(pages), (np.arange(a.pages + 1) * 1030).astype(np.int64))
        q, qoff = unit(24), np.array([0, 24], dtype=np.int32)
        ids = rng.choice(a.pages, 10, replace=False).astype(np.int64)[None, :]
        out["shapes"]["colpali_10_pages"] = measure(
            {"align": lambda: idx.maxsim_align(q, qoff, ids), "subset": lambda: idx.maxsim_subset(q, qoff, ids),
             "numpy": lambda: numpy_align(q, qoff, ids, pages)}, same_dist)
        page = int(ids[0, 0])
        out["shapes"]["colpali_one_map"] = measure(
            {"map": lambda: idx.maxsim_map(q, qoff, [0], [page])[0], "map_numpy": lambda: q @ pages[page].T},
            lambda got: got["map"].shape == got["map_numpy"].shape and bool(np.allclose(got["map"], got["map_numpy"], atol=1e-5)))
    print(f"# d = {d}; best of {a.repeats}, ms per call (host clock, calls complete on return)")
    for name, r in out["shapes"].items():
        cells = "  ".join(f"{k[:-3]} {r[k]:.3f}" for k in r if k.endswith("_ms"))
        ratio = f"  align/subset {r['align_ms'] / r['subset_ms']:.2f}" if "align_ms" in r else ""
        print(f"# {name:>18}  {cells}{ratio}  agree {r['results_agree']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
