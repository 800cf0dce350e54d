"""CPU: sparse search within a listed subset -- the reference (tests/sparse_subset_ref.py) against the contract as a scalar
loop, the new ABI names, the Mi355Index signatures, the service's `within` / `bm25_score_candidates` over a host stand-in, and
the documents' out-of-scope sentences.  No GPU."""

import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import sparse_ref
import sparse_subset_ref as ref
from helpers import OracleIndex, build_golden_stores

ROOT = Path(__file__).resolve().parent.parent
SUBSET_SYMBOLS = ["mi355dr_search_sparse_subset", "mi355dr_search_sparse_subset_device", "mi355dr_search_bm25_subset",
                  "mi355dr_search_bm25_subset_device", "mi355dr_score_sparse_subset", "mi355dr_score_bm25_subset"]


# ---- the reference against the contract as a scalar loop ----------------------------------------------------------------

def _small_corpus(rng, n=60, vocab=40):
    docs = [rng.integers(0, vocab, size=int(rng.integers(1, 30))).tolist() for _ in range(n)]
    docs[7] = []
    docs[20] = list(docs[19])  # identical documents: the id decides
    return sparse_ref.SparseCorpus(docs)


def test_reference_equals_the_scalar_loop():
    rng = np.random.default_rng(5)
    corpus = _small_corpus(rng)
    n = len(corpus)
    for k1, b, off in ((1.2, 0.75, 0), (0.0, 0.0, 1000), (2.0, 1.0, 0)):
        for trial in range(8):
            terms = rng.choice(45, size=int(rng.integers(1, 12)), replace=False).tolist()   # some never occur
            weights = rng.standard_normal(len(terms)).tolist()
            listed = rng.choice(n, size=int(rng.integers(1, n)), replace=False).tolist() + [7, 19, 20]
            raw = [g + off for g in listed] + [-1, off - 1, off + n, listed[0] + off]     # padding, out of range, a duplicate
            rng.shuffle(raw)
            scalar = sparse_ref.score_scalar(corpus, terms, weights, k1, b)                 # statistics of the WHOLE corpus
            want = sorted(((d, i) for i, d in scalar.items() if i in set(listed)))
            for k in (1, 5, n):
                dist, rows = ref.search_weighted_subset(corpus, [(terms, weights)], k, raw, k1, b, off)
                m = min(k, len(want))
                assert rows[0, :m].tolist() == [i + off for _, i in want[:m]] and (rows[0, m:] == -1).all()
                assert dist[0, :m].tolist() == [d for d, _ in want[:m]] and np.isnan(dist[0, m:]).all()   # bit for bit
                assert 7 + off not in rows[0].tolist()
            pool = np.array([raw[:9], raw[-9:]], dtype=np.int64)
            got = ref.score_weighted_subset(corpus, [(terms, weights)] * 2, pool, k1, b, off)
            for q in range(2):
                for j, g in enumerate(pool[q].tolist()):
                    if g - off in scalar and 0 <= g - off < n:
                        assert got[q, j] == scalar[g - off]
                    else:
                        assert np.isnan(got[q, j])
            assert ref.postings_scored(corpus, [(terms, weights)], raw, off) == sum(
                corpus.docs[i].count(t) > 0 for i in set(listed) for t in terms)


def test_reference_edges():
    rng = np.random.default_rng(6)
    corpus = _small_corpus(rng)
    q = [([1, 2, 3], [1.0, 1.0, 1.0])]
    for listed in ([], [-1, -5, 60, 10**12]):
        d, r = ref.search_weighted_subset(corpus, q, 4, listed)
        assert (r == -1).all() and np.isnan(d).all()
    every = list(range(len(corpus)))
    full = sparse_ref.search_weighted(corpus, q, 10)
    got = ref.search_weighted_subset(corpus, q, 10, every)
    assert np.array_equal(full[1], got[1]) and np.array_equal(full[0], got[0], equal_nan=True)
    # BM25: the weights are the whole corpus's, whatever is listed
    tokens = [[3, 3, 5, 44, 1 << 21]]
    d, r = ref.search_bm25_subset(corpus, tokens, 3, every[::2])
    fd, fr = sparse_ref.search_bm25(corpus, tokens, len(corpus))
    keep = [i for i, x in enumerate(fr[0].tolist()) if x >= 0 and x % 2 == 0][:3]
    assert r[0, :len(keep)].tolist() == fr[0, keep].tolist() and d[0, :len(keep)].tolist() == fd[0, keep].tolist()
    assert ref.score_weighted_subset(corpus, q, np.zeros((1, 0), dtype=np.int64)).shape == (1, 0)
    empty = sparse_ref.SparseCorpus([[], []])
    d, r = ref.search_weighted_subset(empty, q, 3, [0, 1])
    assert (r == -1).all() and np.isnan(d).all()


# ---- the ABI names and the Python signatures -------------------------------------------------------------------------------

def test_subset_symbols_are_declared_and_bound(native_built):
    from autorag_research_amd import _native

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mi355dr.h").read_text(), flags=re.S)
    lib = _native.load()
    want_args = {"mi355dr_search_sparse_subset": 12, "mi355dr_search_sparse_subset_device": 13, "mi355dr_search_bm25_subset": 11,
                 "mi355dr_search_bm25_subset_device": 12, "mi355dr_score_sparse_subset": 10, "mi355dr_score_bm25_subset": 9}
    for name in SUBSET_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _native.ABI_SYMBOLS, name
        assert len(getattr(lib, name).argtypes) == want_args[name], name


def test_index_signatures():
    from autorag_research_amd.index import Mi355Index

    sig = lambda name: list(inspect.signature(getattr(Mi355Index, name)).parameters)  # noqa: E731
    assert sig("search_sparse_subset") == ["self", "terms", "weights", "offsets", "k", "doc_ids", "k1", "b", "device_out"]
    assert sig("search_bm25_subset") == ["self", "token_lists", "k", "doc_ids", "k1", "b", "device_out", "offsets"]
    assert sig("score_sparse_subset") == ["self", "terms", "weights", "offsets", "doc_ids", "k1", "b"]
    assert sig("score_bm25_subset") == ["self", "token_lists", "doc_ids", "k1", "b", "offsets"]
    for name in ("search_sparse_subset", "search_bm25_subset", "score_sparse_subset", "score_bm25_subset"):
        p = inspect.signature(getattr(Mi355Index, name)).parameters
        assert p["k1"].default == 1.2 and p["b"].default == 0.75
    assert inspect.signature(Mi355Index.search_bm25_subset).parameters["device_out"].default is False


# ---- the service over the stand-in --------------------------------------------------------------------------------------------

@ref.sparse_subset_methods
class SubsetOracleIndex(OracleIndex):
    """the stand-in of tests/helpers.py with the sparse and the *_subset methods answered by the references"""


@sparse_ref.sparse_methods
class PlainOracleIndex(OracleIndex):
    """a stand-in without the *_subset methods: the service must take its fallback"""


def _service(monkeypatch, cls):
    import autorag_research_amd.service as service

    monkeypatch.setattr(service, "Mi355Index", cls)
    store, g = build_golden_stores()
    return service.Mi355RetrievalService(lambda: store), store, g


@pytest.mark.parametrize("cls", [SubsetOracleIndex, PlainOracleIndex])
def test_service_within(monkeypatch, oracle, cls):
    s, store, g = _service(monkeypatch, cls)
    try:
        for fn, first in ((s.bm25_search, "query_ids"), (s.bm25_search_by_text, "query_text")):
            p = inspect.signature(fn).parameters
            assert list(p)[:4] == [first, "top_k", "tokenizer", "index_name"] and list(p)[-1] == "within"
            assert p["within"].default is None
        assert hasattr(s._unit("chunk").ensure_sparse("simple"), "search_bm25_subset") == (cls is SubsetOracleIndex)
        ids = list(g["ids"])
        text = g["contents"][3]
        full = s.bm25_search_by_text(text, len(ids))
        assert len(full) > 6
        within = [r["doc_id"] for r in full[1::2]] + ["no such key", ids[0]]
        allowed = set(within)
        # a scoped result equals the filtered full result; unknown keys are ignored
        assert s.bm25_search_by_text(text, 3, within=within) == [r for r in full if r["doc_id"] in allowed][:3]
        assert s.bm25_search_by_text(text, 3, within=within, k1=2.0, b=0.0) == [
            r for r in s.bm25_search_by_text(text, len(ids), k1=2.0, b=0.0) if r["doc_id"] in allowed][:3]
        # fewer listed matches than top_k: shorter lists
        short = s.bm25_search_by_text(text, 10, within=[full[2]["doc_id"], full[0]["doc_id"]])
        assert short == [full[0], full[2]]
        # nothing listed: empty lists; None: today's behaviour
        assert s.bm25_search_by_text(text, 5, within=[]) == [] and s.bm25_search_by_text(text, 5, within=["no such key"]) == []
        assert s.bm25_search_by_text(text, 5, within=None) == full[:5]
        # by query id: one block under one list
        qids = [f"q{i}" for i in range(4)]
        assert s.bm25_search(qids, 4, within=within) == [s.bm25_search_by_text(f"query text {i}", 4, within=within) for i in range(4)]
        assert s.bm25_search(qids, 4, within=[]) == [[], [], [], []]
    finally:
        s.close()


def test_service_score_candidates(monkeypatch, oracle):
    s, store, g = _service(monkeypatch, SubsetOracleIndex)
    try:
        p = inspect.signature(s.bm25_score_candidates).parameters
        assert list(p) == ["query_text", "doc_ids", "tokenizer", "k1", "b"] and p["tokenizer"].default == "simple"
        ids = list(g["ids"])
        text = "3 13 57 zzzz 13"                              # (the contents are "chunk text <i>")
        full = {r["doc_id"]: r["score"] for r in s.bm25_search_by_text(text, len(ids))}
        assert set(full) == {ids[3], ids[13], ids[57]}        # every other chunk holds no query term
        got = s.bm25_score_candidates(text, ids + ["no such key"])
        assert got == full and all(v > 0 for v in got.values())   # the search's scores; keys that do not match are absent
        some = [ids[3], ids[0], ids[3]]
        assert s.bm25_score_candidates(text, some) == {k: full[k] for k in some if k in full}
        assert s.bm25_score_candidates(text, []) == {} and s.bm25_score_candidates(text, ["no such key"]) == {}
        assert s.bm25_score_candidates("zzzz qqqq", ids) == {}
        assert s.bm25_score_candidates(text, ids, k1=2.0, b=0.0) == {
            r["doc_id"]: r["score"] for r in s.bm25_search_by_text(text, len(ids), k1=2.0, b=0.0)}
    finally:
        s.close()


# ---- the documents ---------------------------------------------------------------------------------------------------------------

def test_a_key_filter_is_no_longer_out_of_scope():
    header = (ROOT / "include" / "mi355dr.h").read_text()
    start = header.index("---- sparse store")
    section = header[start:header.index("int mi355dr_add_sparse", start)]
    scope = section[section.index("Out of scope"):]
    assert "a key filter" not in scope and "fusion on the device" in scope
    assert "Within a listed subset" in section and "sparse_subset_pairs_max" in section
    design = (ROOT / "DESIGN.md").read_text()
    assert "Within a listed subset" in design
    for m in re.finditer(r"[Oo]ut of scope", design):
        assert "key filter" not in design[m.start():m.start() + 600], design[m.start():m.start() + 200]
