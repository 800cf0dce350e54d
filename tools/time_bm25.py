"""Time `Mi355Index.search_bm25` on one GPU over a synthetic Zipf corpus, next to tests/sparse_ref.py's vectorised reference.

    python tools/time_bm25.py --docs 1000000 --vocab 100000 --doc-len 60 --queries 1024 --query-terms 8 --repeats 5 [--k 10]

The corpus: `--docs` documents, lengths uniform in [1, 2 * doc-len), tokens drawn from a Zipf law (p ~ 1 / rank) over `--vocab`
terms.  A query is `--query-terms` tokens of one random document, so its terms occur and follow the corpus' law.  One block of
`--queries` queries per call; timed with the host clock around calls that are complete on return (host buffers both ways),
after one warm-up; best and all values are kept.  `--ref-queries` of the block's queries are also answered by the reference on
the same data: its time is printed and the library's lines are compared with it bit for bit.  Prints one JSON line with ms per
block, postings scored per second, the bytes of postings (6 B each) and norms (8 B each) the pass must read, the store's
resident bytes and the time of the layout build (the first search after the add)."""

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

SPARSE_STATS = ["sparse_docs", "sparse_total_len", "sparse_postings", "sparse_vocab", "sparse_postings_scored", "sparse_overflows"]


def zipf_corpus(rng, n: int, vocab: int, doc_len: int):
    """(terms int32 flat, offsets int64 [n + 1], lengths): lengths uniform in [1, 2 * doc_len), tokens Zipf (p ~ 1 / rank)"""
    lengths = rng.integers(1, 2 * doc_len, size=n)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cdf = np.cumsum(1.0 / np.arange(1, vocab + 1))
    terms = np.searchsorted(cdf / cdf[-1], rng.random(int(offsets[-1]))).astype(np.int32).clip(0, vocab - 1)
    return terms, offsets, lengths


def doc_queries(rng, terms, offsets, lengths, B: int, query_terms: int) -> list:
    """B queries of `query_terms` tokens of one random document each"""
    picks = rng.integers(0, len(lengths), size=B)
    return [terms[offsets[d] + rng.integers(0, lengths[d], size=query_terms)].tolist() for d in picks]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--doc-len", type=int, default=60)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--query-terms", type=int, default=8)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-queries", type=int, default=8)
    ap.add_argument("--tile-docs", type=int, default=0, help="option sparse_tile_docs (0: the library's default)")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    import sparse_ref
    from autorag_research_amd import Mi355Index

    rng = np.random.default_rng(a.seed)
    n, B = a.docs, a.queries
    terms, offsets, lengths = zipf_corpus(rng, n, a.vocab, a.doc_len)
    queries = doc_queries(rng, terms, offsets, lengths, B, a.query_terms)

    out = {"docs": n, "vocab": a.vocab, "tokens": int(offsets[-1]), "queries": B, "query_terms": a.query_terms, "k": a.k,
           "repeats": a.repeats, "sparse_tile_docs": a.tile_docs or "default"}
    with Mi355Index(8) as idx:
        if a.tile_docs:
            idx.set_option("sparse_tile_docs", a.tile_docs)
        t0 = time.perf_counter()
        idx.add_sparse(terms, offsets)
        out["add_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        idx.search_bm25(queries[:1], a.k)                        # the first search builds and uploads the term-major layout
        out["layout_build_s"] = round(time.perf_counter() - t0, 3)
        idx.search_bm25(queries, a.k)                            # warm-up of the timed shape
        times = []
        for rep in range(a.repeats):
            if rep == a.repeats - 1:
                idx.reset_stats()
            t0 = time.perf_counter()
            dist, rows = idx.search_bm25(queries, a.k)
            times.append((time.perf_counter() - t0) * 1e3)
        stats = {key: idx.stat(key) for key in SPARSE_STATS}
        out["hbm_bytes_resident"] = idx.stat("hbm_bytes_resident")
    scored = stats["sparse_postings_scored"]
    out["ms_per_block_best"] = round(min(times), 3)
    out["ms_per_block_all"] = [round(t, 3) for t in times]
    out["postings_scored_per_block"] = scored
    out["postings_per_s"] = round(scored / (min(times) * 1e-3))
    out["posting_bytes_per_block"] = scored * 6
    out["posting_and_norm_bytes_per_block"] = scored * 14
    out["gb_per_s_postings_and_norms"] = round(scored * 14 / (min(times) * 1e-3) / 1e9, 2)
    out["stats_of_one_call"] = stats
    if a.ref_queries:
        m = min(a.ref_queries, B)
        t0 = time.perf_counter()
        corpus = sparse_ref.SparseCorpus.from_flat(terms, offsets)
        out["reference_build_s"] = round(time.perf_counter() - t0, 3)
        t0 = time.perf_counter()
        rd, rr = sparse_ref.search_bm25(corpus, queries[:m], a.k)
        out["reference_queries"] = m
        out["reference_ms_per_query"] = round((time.perf_counter() - t0) * 1e3 / m, 3)
        out["same_bits_as_reference"] = bool(np.array_equal(rows[:m], rr)
                                             and np.array_equal(dist[:m].view(np.uint64), rd.view(np.uint64)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
