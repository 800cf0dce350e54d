"""Time the sparse searches within a listed subset on one GPU, over the corpus and queries of tools/time_bm25.py.

    python tools/time_sparse_subset.py [--docs 1000000 --vocab 100000 --doc-len 60 --queries 1024 --k 10 --repeats 5]
                                       [--parts crossover,long,score] [--ref-queries 8]

Host clock around calls that are complete on return, one warm-up, best of `--repeats`, every value kept (the spread).
  crossover  both paths forced (`sparse_subset_pairs_max` = 0: the filtered tile pass; 2048: the pair pass) at m = 64, 256,
             1024, 2048 random ids, queries of 3 / 8 / 24 terms; the two answers are compared bit for bit
  long       m = 1 %, 10 %, 50 %, 100 % of the store through the tile pass, scattered (random ids) and clustered (one run of
             consecutive ids), 8-term queries, next to the unrestricted `search_bm25` block of the same run and to what a caller
             did before: k = 1024 over everything plus a host filter -- with how many queries that left short of k listed results
  score      `score_bm25_subset`, B = queries, m = 100 and 1000, ms per call; with --ref-queries the time of
             tests/sparse_subset_ref.py for that many queries, and the bits compared
Prints one JSON line per part."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))


def timed(call, repeats):
    call()                                                   # warm-up of the timed shape
    times, got = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        got = call()
        times.append((time.perf_counter() - t0) * 1e3)
    return got, {"best_ms": round(min(times), 3), "all_ms": [round(t, 3) for t in times]}


def same(a, b):
    return bool(np.array_equal(a[1], b[1]) and np.array_equal(np.nan_to_num(a[0], nan=7.0).view(np.uint64),
                                                              np.nan_to_num(b[0], nan=7.0).view(np.uint64)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--doc-len", type=int, default=60)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="crossover,long,score")
    ap.add_argument("--ref-queries", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    parts = a.parts.split(",")

    from time_bm25 import doc_queries, zipf_corpus

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n, B, k = a.docs, a.queries, a.k
    terms, offsets, lengths = zipf_corpus(rng, n, a.vocab, a.doc_len)
    queries = {qt: doc_queries(rng, terms, offsets, lengths, B, qt) for qt in (8, 3, 24)}   # (8 first: time_bm25's block)
    head = {"docs": n, "tokens": int(offsets[-1]), "queries": B, "k": k, "repeats": a.repeats}
    with Mi355Index(8) as idx:
        idx.add_sparse(terms, offsets)
        idx.search_bm25(queries[8][:1], k)                   # the layout build
        if "crossover" in parts:
            table = []
            for qt in (3, 8, 24):
                for m in (64, 256, 1024, 2048):
                    if m > n:
                        continue
                    ids = rng.choice(n, size=m, replace=False)
                    row = {"query_terms": qt, "m": m}
                    got = {}
                    for name, pairs_max in (("tile", 0), ("pair", 2048)):
                        idx.set_option("sparse_subset_pairs_max", pairs_max)
                        idx.reset_stats()
                        got[name], row[name] = timed(lambda: idx.search_bm25_subset(queries[qt], k, ids), a.repeats)
                        row[name]["tiles_per_call"] = idx.stat("sparse_subset_tiles") // (a.repeats + 1)
                        row[name]["pairs_per_call"] = idx.stat("sparse_subset_pairs") // (a.repeats + 1)
                    row["same_bits"] = same(got["tile"], got["pair"])
                    table.append(row)
            print(json.dumps(dict(head, part="crossover", rows=table)))
        if "long" in parts:
            idx.set_option("sparse_subset_pairs_max", 0)
            q = queries[8]
            full, t_full = timed(lambda: idx.search_bm25(q, k), a.repeats)
            table = [{"list": "unrestricted search_bm25", **t_full}]
            for pct in (1, 10, 50, 100):
                m = n * pct // 100
                for shape in ("scattered", "clustered"):
                    ids = rng.choice(n, size=m, replace=False) if shape == "scattered" else np.arange(m) + int(rng.integers(0, n - m + 1))
                    idx.reset_stats()
                    got, t = timed(lambda: idx.search_bm25_subset(q, k, ids), a.repeats)
                    row = {"list": f"{pct} % {shape}", "m": m, **t, "tiles_per_call": idx.stat("sparse_subset_tiles") // (a.repeats + 1),
                           "overflows": idx.stat("sparse_overflows")}
                    if pct == 100:
                        row["same_bits_as_unrestricted"] = same(got, full)

                    def workaround():
                        d, r = idx.search_bm25(q, 1024)
                        keep = np.isin(r, ids) & (r >= 0)
                        return d, r, keep
                    (d, r, keep), tw = timed(workaround, max(2, a.repeats // 2))
                    row["k1024_plus_host_filter"] = tw
                    row["workaround_queries_with_fewer_than_k"] = int((keep.sum(axis=1) < k).sum())
                    row["subset_queries_with_fewer_than_k"] = int(((got[1] >= 0).sum(axis=1) < k).sum())
                    table.append(row)
            print(json.dumps(dict(head, part="long", query_terms=8, rows=table)))
        if "score" in parts:
            q = queries[8]
            table = []
            for m in (100, 1000):
                pool = rng.integers(0, n, size=(B, m))
                idx.reset_stats()
                got, t = timed(lambda: idx.score_bm25_subset(q, pool), a.repeats)
                row = {"B": B, "m": m, **t, "matches": int((~np.isnan(got)).sum())}
                if a.ref_queries:
                    import sparse_ref
                    import sparse_subset_ref

                    r = min(a.ref_queries, B)
                    corpus = sparse_ref.SparseCorpus.from_flat(terms, offsets)
                    t0 = time.perf_counter()
                    want = sparse_subset_ref.score_bm25_subset(corpus, q[:r], pool[:r])
                    row["reference_ms_per_query"] = round((time.perf_counter() - t0) * 1e3 / r, 3)
                    row["same_bits_as_reference"] = bool(np.array_equal(np.nan_to_num(got[:r], nan=7.0).view(np.uint64),
                                                                        np.nan_to_num(want, nan=7.0).view(np.uint64)))
                table.append(row)
            print(json.dumps(dict(head, part="score", query_terms=8, rows=table)))


if __name__ == "__main__":
    main()
