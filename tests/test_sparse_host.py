"""CPU: the sparse store's reference, the BM25 tokenizers, the new ABI names, and the BM25 pipeline / service methods over a
host stand-in (tests/sparse_ref.py) -- no GPU."""

import asyncio
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest

import sparse_ref
from helpers import OracleIndex, build_golden_stores

ROOT = Path(__file__).resolve().parent.parent
SPARSE_SYMBOLS = ["mi355dr_add_sparse", "mi355dr_size_sparse", "mi355dr_sparse_df", "mi355dr_search_sparse",
                  "mi355dr_search_sparse_device", "mi355dr_search_bm25", "mi355dr_search_bm25_device"]


# ---- the reference against the contract as a scalar loop ----------------------------------------------------------------

def _small_corpus(rng, n=50, vocab=40):
    docs = [rng.integers(0, vocab, size=int(rng.integers(1, 30))).tolist() for _ in range(n)]
    docs[7] = []
    docs[20] = list(docs[19])  # identical documents: the id decides
    return sparse_ref.SparseCorpus(docs)


def test_reference_equals_the_scalar_loop():
    rng = np.random.default_rng(3)
    corpus = _small_corpus(rng)
    assert corpus.n_live == 49 and len(corpus) == 50
    for k1, b in ((1.2, 0.75), (0.0, 0.0), (2.0, 1.0)):
        for _ in range(8):
            terms = rng.choice(45, size=int(rng.integers(1, 12)), replace=False).tolist()   # some never occur
            weights = rng.standard_normal(len(terms)).tolist()
            want = sparse_ref.score_scalar(corpus, terms, weights, k1, b)
            dist, rows = sparse_ref.search_weighted(corpus, [(terms, weights)], 50, k1, b)
            n = len(want)
            assert 7 not in want
            got = rows[0, :n].tolist()
            assert sorted(got) == sorted(want) and (rows[0, n:] == -1).all() and np.isnan(dist[0, n:]).all()
            assert [dist[0, i] for i in range(n)] == [want[r] for r in got]                    # bit for bit (no NaN here)
            assert got == [r for r, _ in sorted(want.items(), key=lambda kv: (kv[1], kv[0]))]  # distance asc, id asc


def test_reference_bm25_layer():
    rng = np.random.default_rng(4)
    corpus = _small_corpus(rng)
    q = [3, 3, 5, 44, 5, 1 << 21, -2]  # repeats count once; unseen and out-of-range terms are dropped
    terms, weights = sparse_ref.bm25_weights(corpus, q)
    assert terms == [3, 5]
    N = corpus.n_live
    assert weights == [math.log(1.0 + ((N - corpus.df(t)) + 0.5) / (corpus.df(t) + 0.5)) for t in terms]
    d1, r1 = sparse_ref.search_bm25(corpus, [q, [], [44]], 5)
    d2, r2 = sparse_ref.search_weighted(corpus, [(terms, weights), ([], []), ([], [])], 5)
    assert np.array_equal(r1, r2) and np.array_equal(d1, d2, equal_nan=True)
    assert (r1[1:] == -1).all() and np.isnan(d1[1:]).all()
    # an empty store answers NaN / -1
    d, r = sparse_ref.search_bm25(sparse_ref.SparseCorpus([[], []]), [[1]], 3)
    assert (r == -1).all() and np.isnan(d).all()


# ---- tokenizers ----------------------------------------------------------------------------------------------------------

def test_simple_tokenizer():
    from autorag_research_amd import bm25

    text = "The quick brown fox -- the QUICK one, 42 times; naïve_under_score"
    ids = bm25.simple_tokenizer(text)
    assert ids == bm25.simple_tokenizer(text) == bm25.get_tokenizer("simple")(text)
    assert all(0 <= i < 2 ** 20 for i in ids)
    assert ids[0] == ids[4] and ids[1] == ids[5]           # lowercased, punctuation is no token
    assert len(ids) == len(re.findall(r"[0-9a-z]+", text.lower()))
    assert bm25.simple_tokenizer("") == [] and bm25.simple_tokenizer("--- !!!") == []
    f = lambda t: [1, 2]  # noqa: E731
    assert bm25.get_tokenizer(f) is f


def test_hub_names_are_refused_without_any_network_call(monkeypatch):
    import socket

    from autorag_research_amd import bm25

    def no_network(*a, **kw):
        raise AssertionError("a network call was attempted")

    monkeypatch.setattr(socket, "create_connection", no_network)
    monkeypatch.setattr(socket.socket, "connect", no_network)
    for name in ("bert", "bert-base-uncased", "wiki_tocken"):
        with pytest.raises(ValueError, match="local directory"):
            bm25.get_tokenizer(name)
    store, _ = build_golden_stores()
    with pytest.raises(ValueError, match="local directory"):
        bm25.Mi355BM25RetrievalPipeline(lambda: store, "bm25_bert", tokenizer="bert")


# ---- the ABI names ---------------------------------------------------------------------------------------------------------

def test_sparse_symbols_are_declared_and_bound(native_built):
    from autorag_research_amd import _native
    from autorag_research_amd.index import Mi355Index

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mi355dr.h").read_text(), flags=re.S)
    lib = _native.load()
    for name in SPARSE_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _native.ABI_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    for method in ("add_sparse", "size_sparse", "sparse_df", "search_sparse", "search_bm25"):
        assert callable(getattr(Mi355Index, method))
    assert inspect.signature(Mi355Index.search_bm25).parameters["device_out"].default is False


# ---- the pipeline and the service over the stand-in ------------------------------------------------------------------------

@sparse_ref.sparse_methods
class SparseOracleIndex(OracleIndex):
    """the stand-in of tests/helpers.py with the sparse methods answered by tests/sparse_ref.py"""


@pytest.fixture()
def store_svc(monkeypatch, oracle):
    import autorag_research_amd.service as service

    monkeypatch.setattr(service, "Mi355Index", SparseOracleIndex)
    store, g = build_golden_stores()
    return store, g


def _expected(store, text, top_k, k1=1.2, b=0.75):
    """what the service must answer for one query text: the reference over the tokenised contents, as result dicts"""
    from autorag_research_amd.bm25 import simple_tokenizer

    table = store.chunks
    corpus = sparse_ref.SparseCorpus([[] if c is None else simple_tokenizer(c) for c in table.contents])
    dist, rows = sparse_ref.search_bm25(corpus, [simple_tokenizer(text)], top_k, k1, b)
    return [{"doc_id": table.ids[r], "score": -d, "content": table.contents[r]} for d, r in zip(dist[0].tolist(), rows[0].tolist()) if r >= 0]


def test_service_bm25_methods(store_svc):
    import autorag_research_amd.service as service

    store, g = store_svc
    s = service.Mi355RetrievalService(lambda: store)
    try:
        # the reference's signatures (orm/service/retrieval_pipeline.py:398-465): names, order, top_k / index_name defaults
        for fn, first in ((s.bm25_search, "query_ids"), (s.bm25_search_by_text, "query_text")):
            p = inspect.signature(fn).parameters
            assert list(p)[:4] == [first, "top_k", "tokenizer", "index_name"]
            assert p["top_k"].default == 10 and p["index_name"].default == "idx_chunk_bm25"
        text = g["contents"][3]
        res = s.bm25_search_by_text(text, 5)
        assert res == _expected(store, text, 5) and len(res) == 5
        assert res[0]["doc_id"] == g["ids"][3]
        scores = [r["score"] for r in res]
        assert all(x > 0 for x in scores) and scores == sorted(scores, reverse=True)   # positive, higher is better
        assert all(r["content"] is not None for r in res)
        # by query id: one block, the same dicts as the by-text form
        qids = [f"q{i}" for i in range(6)]
        out = s.bm25_search(qids, 4)
        assert out == [s.bm25_search_by_text(f"query text {i}", 4) for i in range(6)]
        assert s.bm25_search([], 4) == []
        assert s.bm25_search_by_text("zzzz qqqq", 4) == []          # no term occurs: no match
        with pytest.raises(ValueError, match="Query nope not found"):
            s.bm25_search(["q0", "nope"], 4)
        # other parameters reach the search
        assert s.bm25_search_by_text(text, 5, k1=2.0, b=0.0) == _expected(store, text, 5, 2.0, 0.0)
        # the store is rebuilt whole when the contents change under a refresh
        u = s._unit("chunk")
        first = u.sparse
        assert first is not None and s._unit("chunk").ensure_sparse("simple") is first
        import copy

        table = copy.copy(u.table)
        table.contents = list(u.table.contents)
        table.contents[0] = "entirely new words here"
        s.refresh_unit("chunk", table)
        got = s.bm25_search_by_text("entirely new words", 3)
        assert u.sparse is not first and got and got[0]["doc_id"] == g["ids"][0]
    finally:
        s.close()


def test_pipeline_contract_and_hybrid_child(store_svc):
    from autorag_research_amd.bm25 import Mi355BM25PipelineConfig, Mi355BM25RetrievalPipeline
    from autorag_research_amd.hybrid import Mi355HybridRRFRetrievalPipeline, rrf_fuse
    from autorag_research_amd.pipelines import Mi355VectorSearchRetrievalPipeline

    store, g = store_svc
    cfg = Mi355BM25PipelineConfig(name="bm25_simple")
    assert cfg.get_pipeline_class() is Mi355BM25RetrievalPipeline
    assert cfg.get_pipeline_kwargs() == {"tokenizer": "simple", "index_name": "idx_chunk_bm25", "k1": 1.2, "b": 0.75, "device": 0}
    p = Mi355BM25RetrievalPipeline(lambda: store, "bm25_simple", **{k: v for k, v in cfg.get_pipeline_kwargs().items()})
    dense = Mi355VectorSearchRetrievalPipeline(lambda: store, "dense")
    try:
        assert p.retrieval_unit == "chunk"
        assert p._get_pipeline_config() == {"type": "bm25", "retrieval_unit": "chunk", "tokenizer": "simple",
                                            "index_name": "idx_chunk_bm25", "k1": 1.2, "b": 0.75}
        by_id = asyncio.run(p._retrieve_by_id("q2", 5))
        by_text = asyncio.run(p._retrieve_by_text("query text 2", 5))
        assert by_id == by_text == _expected(store, "query text 2", 5)
        with pytest.raises(ValueError, match="not found"):
            asyncio.run(p._retrieve_by_id("nope", 5))
        # a page as one block; the query that cannot be scored fails alone
        page = p._retrieve_block(["q0", "nope", "q3"], 5)
        assert page[1] is None and page[0] == _expected(store, "query text 0", 5) and page[2] == _expected(store, "query text 3", 5)
        # child 2 of a hybrid: RRF of the dense lists and the BM25 lists
        h = Mi355HybridRRFRetrievalPipeline(lambda: store, "hybrid_own_bm25", dense, p)
        try:
            assert h.retrieval_unit == "chunk"
            fused = h._retrieve_block(["q1", "q4"], 3)
            for qid, got in zip(["q1", "q4"], fused):
                a = asyncio.run(dense._retrieve_by_id(qid, 6))
                b = asyncio.run(p._retrieve_by_id(qid, 6))
                assert got == rrf_fuse(a, b, 60, 3, 6) and len(got) == 3
            assert asyncio.run(h._retrieve_by_id("q1", 3)) == fused[0]
        finally:
            h.close()
    finally:
        p.close()
        dense.close()
