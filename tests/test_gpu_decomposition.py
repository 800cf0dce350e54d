"""GPU: the question-decomposition pipeline over the package's in-memory store and the real index, against the reference's
`_retrieve_by_id` / `_retrieve_by_text` dicts of tests/golden/decomposition_golden.json: doc ids in the golden's order, scores
under the comparison rule tests/test_host_logic.py applies to hyde_golden.json (`_same`: ids, contents, |score diff| <= 1e-12).
The stand-in LLM / embedding / reranker behave like the ones the golden was generated with."""

import asyncio
import json
from pathlib import Path

import numpy as np
import pytest
from helpers import build_golden_stores
from test_host_logic import _same

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


class Msg:
    def __init__(self, content):
        self.content = content


class FakeEmbedding:  # tests/golden/make_golden.py: hyde_fake_models
    def __init__(self):
        self.asked = []

    @staticmethod
    def vec(text):
        seed = sum((i + 1) * b for i, b in enumerate(text.encode())) % (2**32)
        return [float(x) for x in np.random.default_rng(seed).standard_normal(32).astype(np.float32)]

    async def aembed_query(self, text):
        self.asked.append(text)
        return self.vec(text)


class BatchEmbedding(FakeEmbedding):
    def embed_queries(self, texts):
        self.asked.append(list(texts))
        return [self.vec(t) for t in texts]


class FakeReranker:  # tests/golden/make_golden_decomposition.py
    model_name = "fake-reranker"

    def __init__(self):
        self.seen = []

    @staticmethod
    def score(text):
        return (sum((i + 1) * b for i, b in enumerate(text.encode())) % 997) / 997.0

    async def arerank(self, query, documents, top_k=None):
        self.seen.append(list(documents))
        ranked = []
        for i, d in enumerate(documents):
            r = Msg(d)
            r.index, r.text, r.score = i, d, self.score(d)
            ranked.append(r)
        return sorted(ranked, key=lambda r: r.score, reverse=True)[:top_k]


class PlainChild:
    """The dense pipeline behind a plain retrieval-pipeline surface: not one of the package's vector-search classes, so the
    wrapper takes its generic path (child page, `retrieve`, host merge)."""

    retrieval_unit = "chunk"

    def __init__(self, dense):
        self.name, self._dense, self.pipeline_id = "plain", dense, dense.pipeline_id

    async def _retrieve_by_id(self, query_id, top_k):
        return await self._dense._retrieve_by_id(query_id, top_k)

    async def _retrieve_by_text(self, text, top_k):
        return await self._dense._retrieve_by_text(text, top_k)

    async def retrieve(self, text, top_k=10):
        return await self._dense.retrieve(text, top_k)


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLDEN / "decomposition_golden.json").read_text())


@pytest.fixture()
def env(native_built, gold):
    from autorag_research_amd.decompose import Mi355QuestionDecompositionRetrievalPipeline
    from autorag_research_amd.pipelines import Mi355VectorSearchRetrievalPipeline

    store, _ = build_golden_stores()

    class FakeLLM:
        def __init__(self):
            self.asked = []

        async def ainvoke(self, prompt):
            self.asked.append(prompt.split("Question: ")[1].split("\n")[0])
            if self.asked[-1] == "query text 1" and getattr(self, "name_a_stored_query_without_embedding", False):
                return Msg("no embedding")   # the contents of the stored query q_noemb
            return Msg(gold["decomposition"].replace("{query}", prompt.split("Question: ")[1].split("\n")[0]))

    def make(embedding=None, reranker=None, plain=False, name="qd"):
        emb = embedding or FakeEmbedding()
        dense = Mi355VectorSearchRetrievalPipeline(lambda: store, "vs_single", search_mode="single", embedding_model=emb)
        inner = PlainChild(dense) if plain else dense
        p = Mi355QuestionDecompositionRetrievalPipeline(lambda: store, name, FakeLLM(), inner, reranker=reranker)
        assert p._device_path(5) is (not plain) and p.retrieval_unit == "chunk"
        return p, emb

    return make


def test_per_query_forms_match_the_reference(env, gold):
    p, emb = env()
    for flows in (gold["by_id"], gold["by_id_k1"]):
        for qid, g in flows.items():
            _same(asyncio.run(p._retrieve_by_id(qid, g["top_k"])), g["results"])
    # "query text 3" is a stored query: its stored embedding is used, the model is asked for the others only (for q3 the
    # sub-question repeats the question and is dropped, which lets "one too many" in under the cap)
    assert "query text 3" not in emb.asked
    assert set(emb.asked) == {"What is late interaction?", "how are chunks scored", "one too many"}
    g = gold["by_text"]
    _same(asyncio.run(p._retrieve_by_text(g["text"], g["top_k"])), g["results"])
    with pytest.raises(ValueError, match="not found"):
        asyncio.run(p._retrieve_by_id("nope", 5))
    stat = p._inner_retrieval_pipeline._service._unit("chunk").single.stat
    assert stat("group_searches") == 6 and stat("group_subqueries") == 6 * 4   # the question and three sub-questions each


def test_block_equals_the_per_query_form(env, gold):
    for embedding in (FakeEmbedding(), BatchEmbedding()):
        p, emb = env(embedding)
        qids = ["q0", "q2", "nope", "q3", "q_noemb", "q5", "q4"]
        ix = p._inner_retrieval_pipeline._service._unit("chunk").ensure_single()
        before = ix.stat("group_searches")
        block = p._retrieve_block(qids, 5)
        assert ix.stat("group_searches") == before + 1                        # ONE grouped call for the page
        assert block[2] is None and block[4] is None
        for qid, blk in zip(qids, block):
            if blk is not None:
                assert blk == asyncio.run(p._retrieve_by_id(qid, 5))
            if qid in gold["by_id"]:
                _same(blk, gold["by_id"][qid]["results"])
        if isinstance(emb, BatchEmbedding):   # the page's fresh sub-questions in one batch
            assert isinstance(emb.asked[0], list) and len(emb.asked[0]) == 2 * 4 + 3   # (q3: three fresh ones)
    stats = p.run(top_k=5, batch_size=4)
    assert stats["failed_queries"] == ["q_noemb"] and stats["total_queries"] == 6 and stats["total_results"] == 30


def test_a_sub_question_without_embedding_fails_its_query_alone(env, gold):
    """The page form: q3 alone asks "one too many" (its third line repeats the question), and q1's decomposition names a
    stored query that has no embedding.  Both fail alone, in the page's ONE grouped call, and no decomposition is asked for
    twice."""
    class Picky(FakeEmbedding):
        async def aembed_query(self, text):
            if text == "one too many":
                raise RuntimeError("the model fails on this text")
            return await super().aembed_query(text)

    class PickyBatch(Picky, BatchEmbedding):
        def embed_queries(self, texts):
            if "one too many" in texts:
                raise RuntimeError("the model fails on this text")
            return super().embed_queries(texts)

    qids = ["q0", "q3", "q2", "q1", "q5"]
    for embedding in (Picky(), PickyBatch()):
        p, _ = env(embedding)
        p._llm.name_a_stored_query_without_embedding = True
        ix = p._inner_retrieval_pipeline._service._unit("chunk").ensure_single()
        before = ix.stat("group_searches")
        block = p._retrieve_block(qids, 5)
        assert ix.stat("group_searches") == before + 1
        assert sorted(p._llm.asked) == [f"query text {q[1:]}" for q in sorted(qids)]
        assert block[1] is None and block[3] is None
        for qid, blk in zip(qids, block):
            if blk is not None:
                _same(blk, gold["by_id"][qid]["results"])
        for qid in ("q3", "q1"):   # the per-query form raises what the page form reports as that query's failure
            with pytest.raises((RuntimeError, ValueError)):
                asyncio.run(p._retrieve_by_id(qid, 5))


def test_shapes_beyond_the_grouped_caps_take_the_generic_path(env, gold):
    """Five lists of top_k * 2: 4000 entries fit the grouped call (4096), 4500 do not and go the generic way -- answered all
    the same, as the plain child's wrapper answers them.  A list longer than 1024 does not fit either."""
    device, _ = env()
    plain, _ = env(plain=True, name="qd_plain_caps")
    assert device._device_path(512) and not device._device_path(513) and not device._device_path(0)   # 4 lists of 1024
    device.max_subquestions = plain.max_subquestions = 4
    assert device._device_path(409) and not device._device_path(410)                                    # 5 lists: 4090, 4100
    ix = device._inner_retrieval_pipeline._service._unit("chunk").ensure_single()
    for top_k, grouped in ((400, 1), (450, 0)):
        before = ix.stat("group_searches")
        got = asyncio.run(device._retrieve_by_id("q0", top_k))
        assert ix.stat("group_searches") == before + grouped
        assert got == asyncio.run(plain._retrieve_by_id("q0", top_k)) and len(got) > 5
        assert device._retrieve_block(["q0", "nope", "q2"], top_k)[::2] == [got, asyncio.run(plain._retrieve_by_id("q2", top_k))]
        assert ix.stat("group_searches") == before + 2 * grouped
    rr = FakeReranker()
    reranked, _ = env(reranker=rr, name="qd_rr_caps")
    reranked.max_subquestions = 4
    for top_k in (400, 450):   # with a reranker the union is asked for whole: 4000 fits, 4500 goes the generic way
        assert len(asyncio.run(reranked._retrieve_by_id("q1", top_k))) == len(rr.seen[-1]) == len(rr.seen[0]) > 5


def test_generic_path_equals_the_device_path(env, gold):
    device, _ = env()
    generic, _ = env(plain=True, name="qd_plain")
    qids = list(gold["by_id"]) + ["q1"]
    for qid, blk_d, blk_g in zip(qids, device._retrieve_block(qids, 5), generic._retrieve_block(qids, 5)):
        assert blk_d == blk_g == asyncio.run(generic._retrieve_by_id(qid, 5))
        if qid in gold["by_id"]:
            _same(blk_g, gold["by_id"][qid]["results"])
    g = gold["by_text"]
    assert asyncio.run(generic._retrieve_by_text(g["text"], 5)) == asyncio.run(device._retrieve_by_text(g["text"], 5))


def test_reranker_sees_the_whole_union(env, gold):
    g = gold["reranked"]["q1"]
    for plain in (False, True):
        rr = FakeReranker()
        p, _ = env(reranker=rr, plain=plain, name=f"qd_rr_{plain}")
        assert p._get_pipeline_config()["reranker_model"] == "fake-reranker"
        _same(asyncio.run(p._retrieve_by_id("q1", g["top_k"])), g["results"])
        assert rr.seen == [g["documents"]] and len(g["documents"]) == len(g["union_ids"]) > g["top_k"]
        blk = p._retrieve_block(["q1"], g["top_k"])[0]
        _same(blk, g["results"])
        assert rr.seen[1] == g["documents"]


def test_service_groups_in_multi_mode(native_built):
    """vector_search_groups, multi mode: the merge of the sub-queries' `maxsim_search_by_embeddings` lists by best score"""
    from autorag_research_amd.decompose import merge_results
    from autorag_research_amd.service import Mi355RetrievalService

    store, g = build_golden_stores()
    s = Mi355RetrievalService(lambda: store)
    Qm = [np.asarray(m, dtype=np.float32) for m in g["Qm"]]
    groups = [[Qm[0], Qm[1], Qm[2]], [Qm[3]], [], [Qm[4], np.zeros((0, 8), np.float32), Qm[5]]]
    for top_k, fetch_k in ((5, 8), (12, 6)):
        got = s.vector_search_groups(groups, top_k, fetch_k, search_mode="multi")
        for grp, res in zip(groups, got):
            lists = s.maxsim_search_by_embeddings(grp, fetch_k) if grp else []
            want = merge_results(lists)
            if len(want) > top_k:
                assert want[top_k - 1]["score"] != want[top_k]["score"]
            assert res == want[:top_k]
    s.close()
