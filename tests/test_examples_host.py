"""CPU: the declaration and binding of the six entry points of the search by examples / feedback, the wrappers' list
handling, and the service methods and the feedback pipeline over a stand-in index that answers from tests/examples_ref.py."""

import asyncio
import re
from pathlib import Path

import numpy as np
import pytest

import examples_ref as xr
from helpers import OracleIndex, build_golden_stores

ROOT = Path(__file__).resolve().parent.parent
NAN = float("nan")
NAMES = ("mi355dr_combine_rows", "mi355dr_combine_rows_device", "mi355dr_search_examples", "mi355dr_search_examples_device",
         "mi355dr_search_feedback", "mi355dr_search_feedback_device")


# ---- the ABI and its binding ---------------------------------------------------------------------------------------------------

def test_header_declares_and_native_binds_the_six_entry_points(native_built):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mi355dr.h").read_text(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    assert re.search(r"#define\s+MI355DR_EXAMPLES_KEEP\s+1\b", text)
    from autorag_research_amd import _native

    assert set(NAMES) <= set(_native.ABI_SYMBOLS)
    lib = _native.load()
    assert [len(getattr(lib, name).argtypes) for name in NAMES] == [12, 13, 14, 15, 9, 10]


def test_wrappers_pad_ragged_lists_and_check_shapes_before_the_library():
    from autorag_research_amd.index import Mi355Index

    pad = Mi355Index._example_lists
    assert pad([[1, 2, 3], [4], []], 3).tolist() == [[1, 2, 3], [4, -1, -1], [-1, -1, -1]]
    assert pad([7, 8], None).tolist() == [[7, 8]]                   # a flat list: one slot
    assert pad(None, 4).shape == (4, 0) and pad((), 4).shape == (4, 0)
    assert pad(np.array([[1, 2]], dtype=np.int32), 1).dtype == np.int64
    with pytest.raises(ValueError):
        pad([[1], [2]], 3)

    class Unreached(Mi355Index):   # (no handle: the checks come before the first use of the library)
        def __init__(self):
            self.dim = 4

        def __del__(self):
            pass

    ix = Unreached()
    with pytest.raises(ValueError):
        ix.search_examples([[1, 2]], 3, queries=np.zeros((2, 4), np.float32))      # one list, two base vectors
    with pytest.raises(ValueError):
        ix.combine_rows([[1], [2]], [[3]])                                         # two slots, one list of negatives
    with pytest.raises(ValueError):
        ix.search_feedback(np.zeros((2, 5), np.float32), 3)


# ---- the service methods and the pipeline over a stand-in ---------------------------------------------------------------------

class ExamplesOracleIndex(OracleIndex):
    """the stand-in of tests/helpers.py, with the three calls answered by the reference over the oracle's distances"""

    calls = []

    def search_examples(self, pos_ids, k, neg_ids=None, queries=None, alpha=1.0, beta=1.0, gamma=1.0, keep=False):
        pos, neg = np.asarray(pos_ids), np.asarray(neg_ids)
        type(self).calls.append(("search_examples", pos.tolist(), neg.tolist(), k, queries is not None, alpha, beta, gamma, keep))
        return xr.search_examples(self._o, self._rows, queries, pos, neg, alpha, beta, gamma, k, self.metric, self.row_offset,
                                  None, keep)[:2]

    def search_feedback(self, queries, k, fb_k=10, alpha=1.0, beta=0.75):
        type(self).calls.append(("search_feedback", len(queries), k, fb_k, alpha, beta))
        return xr.search_feedback(self._o, self._rows, queries, k, fb_k, alpha, beta, self.metric, self.row_offset)[:2]


@pytest.fixture()
def svc(monkeypatch, oracle):
    import autorag_research_amd.service as service

    monkeypatch.setattr(service, "Mi355Index", ExamplesOracleIndex)
    ExamplesOracleIndex.calls = []
    store, g = build_golden_stores()
    s = service.Mi355RetrievalService(lambda: store)
    yield s, g, store
    s.close()


def test_service_similar_to_examples(svc):
    s, g, _ = svc
    ids = list(g["ids"])
    emb = [float(x) for x in g["Q"][2]]
    out = s.similar_to_examples([ids[4], ids[17], ids[4]], [ids[30]], top_k=6, embedding=emb, alpha=0.5, beta=2.0, gamma=0.25)
    # key -> table position -> index row, in list order, repeats kept
    assert ExamplesOracleIndex.calls == [("search_examples", [[4, 17, 4]], [[30]], 6, True, 0.5, 2.0, 0.25, False)]
    C = np.asarray(g["C"], dtype=np.float32)
    d, r, _ = xr.search_examples(s._unit("chunk").single._o, C, g["Q"][2:3], [[4, 17, 4]], [[30]], 0.5, 2.0, 0.25, 6)
    assert [x["doc_id"] for x in out] == [ids[i] for i in r[0]] and [x["score"] for x in out] == (1.0 - d[0]).tolist()
    assert len(out) == 6 and not {ids[4], ids[17], ids[30]} & {x["doc_id"] for x in out}
    assert all(x["content"] is not None for x in out)
    # without a vector; keep: the chunk is its own nearest
    out = s.similar_to_examples([ids[4]], top_k=3, keep=True)
    assert ExamplesOracleIndex.calls[-1] == ("search_examples", [[4]], [[]], 3, False, 1.0, 1.0, 1.0, True)
    assert out[0]["doc_id"] == ids[4] and out[1:] == s.similar_to_examples([ids[4]], top_k=2)
    assert s.similar_to_examples([], top_k=3) == [] and s.similar_to_examples([], top_k=3, embedding=[]) == []
    # the image unit: no contents
    img = s.similar_to_examples([g["img_ids"][2]], top_k=3, unit="image_chunk")
    assert len(img) == 3 and all(x["content"] is None for x in img) and g["img_ids"][2] not in [x["doc_id"] for x in img]


def test_service_feedback(svc):
    s, g, _ = svc
    ids = list(g["ids"])
    qids = ["q3", "q0", "q3"]
    got = s.vector_search_feedback(qids, top_k=5, fb_k=7, alpha=1.0, beta=0.5)
    assert ExamplesOracleIndex.calls == [("search_feedback", 3, 5, 7, 1.0, 0.5)]
    C = np.asarray(g["C"], dtype=np.float32)
    d, r = xr.search_feedback(s._unit("chunk").single._o, C, g["Q"][[3, 0, 3]], 5, 7, 1.0, 0.5)[:2]
    assert [[x["doc_id"] for x in res] for res in got] == [[ids[i] for i in row] for row in r]
    assert [[x["score"] for x in res] for res in got] == (1.0 - d).tolist() and got[0] == got[2]
    one = s.vector_search_feedback_by_embedding([float(x) for x in g["Q"][0]], top_k=5, fb_k=7, beta=0.5)
    assert one == got[1] and ExamplesOracleIndex.calls[-1] == ("search_feedback", 1, 5, 7, 1.0, 0.5)
    assert s.vector_search_feedback_by_embedding([], top_k=5) == [] and s.vector_search_feedback([]) == []
    assert s.vector_search_feedback(["q1"])[0] == s.vector_search_feedback(["q1"], 10, 10, 1.0, 0.75, "chunk")[0]   # the defaults
    with pytest.raises(ValueError, match="not found"):
        s.vector_search_feedback(["q0", "nope"])
    with pytest.raises(ValueError, match="no embedding"):
        s.vector_search_feedback(["q_noemb"])


def test_service_refusals(monkeypatch, oracle):
    import autorag_research_amd.service as service
    from autorag_research_amd.store import InMemoryStore

    monkeypatch.setattr(service, "Mi355Index", ExamplesOracleIndex)
    ExamplesOracleIndex.calls = []
    rng = np.random.default_rng(5)
    emb = rng.standard_normal((6, 8)).astype(np.float32)
    emb[2] = NAN                                                    # a chunk without a stored embedding
    store = InMemoryStore()
    store.set_chunks([f"c{i}" for i in range(6)], [f"text {i}" for i in range(6)], embedding=emb)
    s = service.Mi355RetrievalService(lambda: store)
    try:
        with pytest.raises(ValueError, match="not found"):
            s.similar_to_examples(["c0", "nope"])
        with pytest.raises(ValueError, match="not found"):
            s.similar_to_examples(["c0"], ["nope"])
        with pytest.raises(ValueError, match="no embedding"):
            s.similar_to_examples(["c2"])
        assert ExamplesOracleIndex.calls == []
        # the index holds the five stored rows: c3 is row 2, and c2 is no result of anything
        out = s.similar_to_examples(["c3"], ["c5"], top_k=10)
        assert ExamplesOracleIndex.calls[0][:4] == ("search_examples", [[2]], [[4]], 10)
        assert sorted(x["doc_id"] for x in out) == ["c0", "c1", "c4"]
        s._world = object()          # a process group: refused before anything is asked of it
        for call in (lambda: s.similar_to_examples(["c0"]), lambda: s.similar_to_examples(["nope"]),
                     lambda: s.vector_search_feedback(["nope"]), lambda: s.vector_search_feedback_by_embedding([0.0] * 8)):
            with pytest.raises(NotImplementedError):
                call()
    finally:
        s._world = None
        s.close()


def test_feedback_pipeline(monkeypatch, oracle):
    import autorag_research_amd.service as service
    from autorag_research_amd.compat import EmbeddingError
    from autorag_research_amd.embeddings import HashingEmbeddings
    from autorag_research_amd.feedback import Mi355FeedbackPipelineConfig, Mi355FeedbackRetrievalPipeline

    monkeypatch.setattr(service, "Mi355Index", ExamplesOracleIndex)
    ExamplesOracleIndex.calls = []
    store, g = build_golden_stores()
    cfg = Mi355FeedbackPipelineConfig(name="fb", fb_k=7, alpha=0.9, beta=0.5)
    assert cfg.get_pipeline_class() is Mi355FeedbackRetrievalPipeline
    assert cfg.get_pipeline_kwargs() == {"embedding_model": None, "fb_k": 7, "alpha": 0.9, "beta": 0.5, "device": 0}
    p = Mi355FeedbackRetrievalPipeline(lambda: store, "fb", **cfg.get_pipeline_kwargs())
    try:
        assert p._get_pipeline_config() == {"type": "mi355_feedback", "retrieval_unit": "chunk", "search_mode": "single",
                                            "fb_k": 7, "alpha": 0.9, "beta": 0.5}
        assert store.pipelines[p.pipeline_id]["config"] == p._get_pipeline_config()
        qids = ["q0", "nope", "q2", "q_noemb", "q5"]
        block = p._retrieve_block(qids, 4)
        assert ExamplesOracleIndex.calls == [("search_feedback", 3, 4, 7, 0.9, 0.5)]             # ONE call for the page
        assert block[1] is None and block[3] is None
        want = p._service.vector_search_feedback(["q0", "q2", "q5"], 4, fb_k=7, alpha=0.9, beta=0.5)
        assert [block[0], block[2], block[4]] == want
        assert asyncio.run(p._retrieve_by_id("q2", 4)) == want[1]
        assert asyncio.run(p.retrieve("query text 5", 4)) == want[2]               # a stored query's text: the id path
        with pytest.raises(EmbeddingError):
            asyncio.run(p.retrieve("unknown text", 3))
        stats = p.run(top_k=4, batch_size=4)
        assert stats["failed_queries"] == ["q_noemb"] and stats["total_queries"] == 6 and stats["total_results"] == 24
        assert store.chunk_results[(p.pipeline_id, "q2")] == [(x["doc_id"], x["score"]) for x in want[1]]
    finally:
        p.close()
    p2 = Mi355FeedbackRetrievalPipeline(lambda: store, "fb2", embedding_model=HashingEmbeddings(32))
    try:
        assert (p2.fb_k, p2.alpha, p2.beta) == (10, 1.0, 0.75)
        res = asyncio.run(p2.retrieve("unknown text", 3))
        assert len(res) == 3 and ExamplesOracleIndex.calls[-1] == ("search_feedback", 1, 3, 10, 1.0, 0.75)
    finally:
        p2.close()
    for bad in ({"fb_k": 0}, {"fb_k": 1025}, {"alpha": -1.0}, {"beta": NAN}, {"beta": float("inf")}):
        with pytest.raises(ValueError):
            Mi355FeedbackRetrievalPipeline(lambda: store, "bad", **bad)
