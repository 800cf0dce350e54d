"""Time `Mi355Index.search_collapsed_device` on one GPU next to the plain search it is built on and the recipe it replaces.

    python tools/time_collapse.py --rows 1000000 --dim 768 --queries 1024 --k 10 --cap 1 --repeats 7

Timed with the host clock around calls that are complete on return, after one warm-up of every shape; the variants alternate
inside every repeat, best and all values are kept.  Two seeded corpora, sources of 8 consecutive rows each:
  gaussian   independent Gaussian rows: the cap almost never bites, a query is finished in the first round
  copies     every source is 8 near-copies of one Gaussian row (the row plus small noise): a query's head is made of runs of 8,
             the k-th kept entry lies about 8 k deep
Per corpus:
  search_K            search_device at k = 10, 128 and 1024, device buffers: the yardstick (the plain entry point)
  collapsed_F         search_collapsed_device at fetch_k = F in 10, 20, 40, 128, 1024 (max_fetch 1024), the key table on the
                      device, with the call's `collapse_researched` next to it
  kernel_F            k_collapse_lists alone over [B, F] device lists, by the index's event timer (timer_start / timer_stop)
  host_walk           what a caller does without it: search at 1024 into host arrays (the download included), the walk in numpy
Also checks that every fetch_k returns the same bits.  Prints one JSON line."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def numpy_walk(rows: np.ndarray, keys: np.ndarray, cap: int, k: int) -> np.ndarray:
    """[B, k] kept rows of ranked lists `rows` [B, f] (-1 padded): rank within the source by one stable sort per list"""
    B, f = rows.shape
    out = np.full((B, k), -1, dtype=np.int64)
    for b in range(B):
        r = rows[b]
        r = r[r >= 0]
        src = keys[r]
        order = np.argsort(src, kind="stable")
        s = src[order]
        start = np.r_[True, s[1:] != s[:-1]]
        first = np.maximum.accumulate(np.where(start, np.arange(s.shape[0]), 0))
        rank = np.empty(s.shape[0], dtype=np.int64)
        rank[order] = np.arange(s.shape[0]) - first
        kept = r[(src < 0) | (rank < cap)][:k]
        out[b, :kept.shape[0]] = kept
    return out


def build(idx, corpus: str, n: int, d: int, rng) -> None:
    chunk = 125_000                                     # a multiple of 8: a source never straddles two chunks
    for r0 in range(0, n, chunk):
        m = min(chunk, n - r0)
        if corpus == "gaussian":
            rows = rng.standard_normal((m, d), dtype=np.float32)
        else:
            base = rng.standard_normal(((m + 7) // 8, d), dtype=np.float32)
            rows = np.repeat(base, 8, axis=0)[:m] + np.float32(0.02) * rng.standard_normal((m, d), dtype=np.float32)
        idx.add(rows)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--cap", type=int, default=1)
    ap.add_argument("--fetch-k", type=int, nargs="+", default=[10, 20, 40, 128, 1024])
    ap.add_argument("--search-k", type=int, nargs="+", default=[10, 128, 1024])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--corpora", nargs="+", default=["gaussian", "copies"])
    a = ap.parse_args()

    from autorag_research_amd import Mi355Index

    n, d, B, k, cap, max_fetch = a.rows, a.dim, a.queries, a.k, a.cap, 1024
    keys = (np.arange(n) // 8).astype(np.int64)
    out = {"rows": n, "dim": d, "queries": B, "k": k, "cap": cap, "max_fetch": max_fetch, "repeats": a.repeats}
    for corpus in a.corpora:
        rng = np.random.default_rng(a.seed)
        Q = rng.standard_normal((B, d), dtype=np.float32)
        with Mi355Index(d) as idx:
            build(idx, corpus, n, d, rng)
            wmax = max(max_fetch, *a.search_k)
            pq, od, orr = idx.dev_alloc(Q.nbytes), idx.dev_alloc(B * wmax * 8), idx.dev_alloc(B * wmax * 8)
            ok_, oc, os_ = idx.dev_alloc(B * k * 8), idx.dev_alloc(B * 4), idx.dev_alloc(B * 4)
            kd, kr = idx.dev_alloc(B * k * 8), idx.dev_alloc(B * k * 8)
            idx.dev_upload(pq, Q)
            with idx.upload_keys(keys) as table:
                def collapsed(f: int):
                    idx.search_collapsed_device(pq, B, k, cap, f, max_fetch, kd, kr, ok_, oc, os_, keys_ptr=table.ptr,
                                                keys_len=table.length)

                def host_walk():
                    _, rows = idx.search(Q, max_fetch)
                    return numpy_walk(rows, keys, cap, k)

                variants = {f"search_{w}": (lambda w=w: idx.search_device(pq, B, w, od, orr)) for w in a.search_k}
                variants.update({f"collapsed_{f}": (lambda f=f: collapsed(f)) for f in a.fetch_k})
                variants["host_walk"] = host_walk
                times = {name: [] for name in variants}
                for rep in range(a.repeats + 1):                  # (repeat 0: warm-up of every shape, not kept)
                    for name, fn in variants.items():
                        t0 = time.perf_counter()
                        fn()
                        if rep:
                            times[name].append((time.perf_counter() - t0) * 1e3)
                    print(f"{corpus}: repeat {rep} done", file=sys.stderr, flush=True)
                res = {name: {"ms_best": round(min(t), 3), "ms_all": [round(x, 3) for x in t]} for name, t in times.items()}
                # the re-searches of one call at each fetch_k, and the bits: the same at every fetch_k, the rows those of the walk
                bits = []
                for f in a.fetch_k:
                    idx.reset_stats()
                    collapsed(f)
                    res[f"collapsed_{f}"]["researched"] = idx.stat("collapse_researched")
                    res[f"collapsed_{f}"]["truncated"] = idx.stat("collapse_truncated")
                    gd, gr = np.empty((B, k)), np.empty((B, k), dtype=np.int64)
                    idx.dev_download(kd, gd)
                    idx.dev_download(kr, gr)
                    bits.append((gd.view(np.uint64).copy(), gr))
                res["same_bits_at_every_fetch_k"] = bool(all(np.array_equal(b[0], bits[0][0]) and np.array_equal(b[1], bits[0][1])
                                                             for b in bits))
                res["rows_equal_host_walk"] = bool(np.array_equal(bits[0][1], host_walk()))
                # the kernel alone, by the event timer, over the lists a search at F left on the device
                for f in a.fetch_k:
                    idx.search_device(pq, B, f, od, orr)
                    best = []
                    for rep in range(a.repeats + 1):
                        idx.timer_start()
                        idx.collapse_lists_device(od, orr, f, B, cap, k, kd, kr, ok_, None, oc, os_, keys_ptr=table.ptr,
                                                  keys_len=table.length)
                        ms = idx.timer_stop()
                        if rep:
                            best.append(ms)
                    res[f"kernel_{f}"] = {"ms_best": round(min(best), 4)}
            for p in (pq, od, orr, ok_, oc, os_, kd, kr):
                idx.dev_free(p)
        out[corpus] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
