"""Time `Mi355Index.set_sparse` and the searches behind it on one GPU, over tools/time_bm25.py's corpus and queries.

    python tools/time_sparse_update.py --replace-pct 1 [--overlay-max-pct 100] [--docs 1000000 --vocab 100000 --doc-len 60
                                       --queries 1024 --query-terms 8 --k 10 --repeats 5]

One store is built (add_sparse + the first search, a full layout build) and its steady block time taken.  Then `--replace-pct`
percent of the documents, drawn at random, are replaced by new documents of the same law in ONE set_sparse, under option
`sparse_overlay_max_pct` = `--overlay-max-pct` (100: whatever the size, the overlay path).  Timed with the host clock around
calls that are complete on return: the set, the first search after it (the overlay -- or full -- build and its upload), and the
steady block time (one warm-up, best of `--repeats`).  Last, what the calls replace: a FRESH store over the same current
documents -- add_sparse of everything, its first search, its steady block time -- whose lines must equal the mutated store's bit
for bit.  Prints one JSON line."""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

BUILD_STATS = ["sparse_full_builds", "sparse_overlay_builds", "sparse_overlay_postings", "sparse_dead_postings", "sparse_postings",
               "sparse_postings_scored", "sparse_overflows", "hbm_bytes_resident"]


def steady(idx, queries, k, repeats):
    idx.search_bm25(queries, k)                                  # warm-up of the timed shape
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = idx.search_bm25(queries, k)
        times.append((time.perf_counter() - t0) * 1e3)
    return [round(t, 3) for t in times], out


def replaced(terms, offsets, ids, new_terms, new_offsets):
    """the flat corpus with documents `ids` replaced: (terms, offsets)"""
    n = len(offsets) - 1
    lengths = np.diff(offsets)
    changed = np.zeros(n, dtype=bool)
    changed[ids] = True
    doc_of = np.repeat(np.arange(n, dtype=np.int64), lengths)
    keep = ~changed[doc_of]
    cat_terms = np.concatenate([terms[keep], new_terms])
    cat_docs = np.concatenate([doc_of[keep], np.repeat(np.asarray(ids, dtype=np.int64), np.diff(new_offsets))])
    order = np.argsort(cat_docs, kind="stable")
    lengths = lengths.copy()
    lengths[ids] = np.diff(new_offsets)
    return cat_terms[order], np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--doc-len", type=int, default=60)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--query-terms", type=int, default=8)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replace-pct", type=float, default=1.0)
    ap.add_argument("--overlay-max-pct", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    from time_bm25 import doc_queries, zipf_corpus

    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n = a.docs
    terms, offsets, lengths = zipf_corpus(rng, n, a.vocab, a.doc_len)
    queries = doc_queries(rng, terms, offsets, lengths, a.queries, a.query_terms)
    m = max(1, round(n * a.replace_pct / 100.0))
    ids = np.sort(rng.choice(n, size=m, replace=False))
    new_terms, new_offsets, _ = zipf_corpus(rng, m, a.vocab, a.doc_len)
    cur_terms, cur_offsets = replaced(terms, offsets, ids, new_terms, new_offsets)

    out = {"docs": n, "tokens": int(offsets[-1]), "queries": a.queries, "query_terms": a.query_terms, "k": a.k,
           "replace_pct": a.replace_pct, "replaced_docs": m, "sparse_overlay_max_pct": a.overlay_max_pct}
    with Mi355Index(8) as idx:
        idx.set_option("sparse_overlay_max_pct", a.overlay_max_pct)
        idx.add_sparse(terms, offsets)
        idx.search_bm25(queries[:1], a.k)
        out["before_ms_per_block"], _ = steady(idx, queries, a.k, a.repeats)
        t0 = time.perf_counter()
        idx.set_sparse(ids, new_terms, new_offsets)
        out["set_s"] = round(time.perf_counter() - t0, 4)
        t0 = time.perf_counter()
        idx.search_bm25(queries[:1], a.k)                        # the first search brings the device layout up to date
        out["first_search_s"] = round(time.perf_counter() - t0, 4)
        out["mutated_ms_per_block"], got = steady(idx, queries, a.k, a.repeats)
        out["mutated_stats"] = {key: idx.stat(key) for key in BUILD_STATS}
    with Mi355Index(8) as fresh:                                 # what the set replaces: everything added again
        t0 = time.perf_counter()
        fresh.add_sparse(cur_terms, cur_offsets)
        out["fresh_add_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        fresh.search_bm25(queries[:1], a.k)
        out["fresh_first_search_s"] = round(time.perf_counter() - t0, 3)
        out["fresh_ms_per_block"], want = steady(fresh, queries, a.k, a.repeats)
        out["fresh_stats"] = {key: fresh.stat(key) for key in BUILD_STATS}
    out["mutated_ms_best"], out["fresh_ms_best"] = min(out["mutated_ms_per_block"]), min(out["fresh_ms_per_block"])
    out["same_bits_as_fresh"] = bool(np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
