"""GPU: the hybrid pipelines' device path -- two searches whose lists stay in HBM, one fusion launch, one [B, top_k] download
-- returns exactly the dicts the host path builds from the children's own answers, fails the same queries alone, runs only
where it should, and persists the same rows.

The store is build_golden_stores() with one chunk without content (an empty BM25 document) and one chunk without an embedding,
so the dense index's rows are NOT table positions behind it and the fusion needs its map."""

import asyncio
import struct

import numpy as np
import pytest

import fuse_ref
from helpers import build_golden_stores

pytestmark = pytest.mark.gpu

QIDS = [f"q{i}" for i in range(6)]
PAGE = ["q0", "q_noemb", "q3", "nope", "q5", "q1"]
TOP_K = 4


@pytest.fixture(scope="module")
def world(native_built):
    from autorag_research_amd.bm25 import Mi355BM25RetrievalPipeline
    from autorag_research_amd.pipelines import Mi355VectorSearchRetrievalPipeline

    store, g = build_golden_stores()
    store.chunks.contents[5] = None
    store.chunks.embedding[7] = np.nan           # NULL embedding: no index row, rows behind it are positions - 1
    dense = Mi355VectorSearchRetrievalPipeline(lambda: store, "dense")
    lex = Mi355BM25RetrievalPipeline(lambda: store, "bm25")
    made = []
    yield store, dense, lex, made
    for p in made + [dense, lex]:
        p.close()


def hybrid(world, kind, order, **kw):
    from autorag_research_amd.hybrid import Mi355HybridCCRetrievalPipeline, Mi355HybridRRFRetrievalPipeline

    store, dense, lex, made = world
    a, b = (dense, lex) if order == "dense-first" else (lex, dense)
    name = f"h{len(made)}"
    if kind == "rrf":
        h = Mi355HybridRRFRetrievalPipeline(lambda: store, name, a, b, **kw)
    else:
        mins = {"pipeline_1_min": -1.0 if a is dense else 0.0, "pipeline_2_min": -1.0 if b is dense else 0.0} if kind == "tmm" else {}
        h = Mi355HybridCCRetrievalPipeline(lambda: store, name, a, b, weight=0.3, normalize_method=kind, **mins, **kw)
    made.append(h)
    return h


def child_answers(h, qid, fetch_k):
    out = []
    for child in (h._retrieval_pipeline_1, h._retrieval_pipeline_2):
        try:
            out.append(asyncio.run(child._retrieve_by_id(qid, fetch_k)))
        except ValueError:
            return None
    return out


def host_page(h, qids, top_k):
    """what today's host path answers: the pipeline's own fuse over the children's `_retrieve_by_id` answers at fetch_k"""
    fetch_k = top_k * h.fetch_k_multiplier
    pages = [child_answers(h, q, fetch_k) for q in qids]
    return [None if ab is None else h._fuse_results(ab[0], ab[1], top_k, fetch_k) for ab in pages]


def fusing_handle(h):
    """the handle the device path fuses on: the first child's"""
    first = h._retrieval_pipeline_1
    unit = first._service._unit("chunk")
    return unit.single if hasattr(first, "search_mode") else unit.sparse


def fused_queries(h):
    ix = fusing_handle(h)
    return 0 if ix is None else ix.stat("fuse_queries")


def bits(page):
    return [None if r is None else [(d["doc_id"], struct.pack("<d", d["score"])) for d in r] for r in page]


@pytest.mark.parametrize("order", ["dense-first", "bm25-first"])
@pytest.mark.parametrize("kind", ["rrf", "mm", "tmm"])
def test_block_equals_the_host_fuse_of_the_childrens_answers(world, kind, order):
    h = hybrid(world, kind, order)
    want = host_page(h, PAGE, TOP_K)
    assert [w is None for w in want] == [False, True, False, True, False, False]
    before = fused_queries(h)
    got = h._retrieve_block(PAGE, TOP_K)
    assert got == want and bits(got) == bits(want)
    assert all(len(r) == TOP_K and set(r[0]) == {"doc_id", "score"} for r in got if r is not None)
    assert fused_queries(h) - before == 4                          # the device path ran, on the first child's handle
    off = hybrid(world, kind, order, device_fusion=False)
    before = fused_queries(off)
    assert bits(off._retrieve_block(PAGE, TOP_K)) == bits(want)
    assert fused_queries(off) == before                            # the host path: the same dicts, no fusion launch


def test_the_dense_map_is_not_the_identity(world):
    _, dense, _, _ = world
    asyncio.run(dense._retrieve_by_id("q0", 2))
    rows = dense._service._unit("chunk").single_rows
    assert rows.shape[0] == 299 and rows[7] == 8


@pytest.mark.parametrize("kind", ["z", "dbsf"])
def test_z_and_dbsf_take_the_device_only_when_asked(world, kind):
    h = hybrid(world, kind, "dense-first")
    want_host = host_page(h, QIDS, TOP_K)
    before = fused_queries(h)
    assert h._retrieve_block(QIDS, TOP_K) == want_host
    assert fused_queries(h) == before                              # None: the host's `** 0.5` and sum() are not the library's
    on = hybrid(world, kind, "dense-first", device_fusion=True)
    got = on._retrieve_block(QIDS, TOP_K)
    assert fused_queries(on) - before == len(QIDS)
    want = [fuse_ref.cc_restated(*child_answers(on, q, 2 * TOP_K), 0.3, kind)[:TOP_K] for q in QIDS]
    assert bits(got) == bits(want)


def test_other_children_take_the_host_path(world):
    from autorag_research_amd.hybrid import Mi355HybridRRFRetrievalPipeline
    from autorag_research_amd.pipelines import Mi355VectorSearchRetrievalPipeline

    store, dense, lex, made = world

    class Recorded:                                                # any object with `_retrieve_by_id`
        name, retrieval_unit = "recorded", "chunk"

        async def _retrieve_by_id(self, query_id, top_k):
            return await dense._retrieve_by_id(query_id, top_k)

    multi = Mi355VectorSearchRetrievalPipeline(lambda: store, "dense-multi", search_mode="multi")
    made.append(multi)
    asyncio.run(dense._retrieve_by_id("q0", 2))
    asyncio.run(lex._retrieve_by_id("q0", 2))
    handles = [dense._service._unit("chunk").single, lex._service._unit("chunk").sparse]
    for first in (Recorded(), multi):
        h = Mi355HybridRRFRetrievalPipeline(lambda: store, f"h-{first.name}", first, lex, device_fusion=True)
        made.append(h)
        before = [ix.stat("fuse_queries") for ix in handles]
        got = h._retrieve_block(QIDS[:3], TOP_K)
        assert bits(got) == bits(host_page(h, QIDS[:3], TOP_K)) and all(len(r) == TOP_K for r in got)
        assert [ix.stat("fuse_queries") for ix in handles] == before and multi._service._unit("chunk").single is None


def test_run_persists_the_same_rows_either_way(world):
    store = world[0]
    rows = {}
    for flag in (None, False):
        h = hybrid(world, "rrf", "dense-first", device_fusion=flag)
        stats = h.run(top_k=3)
        assert stats["total_queries"] == 6                         # (q_noemb has no embedding: it fails alone)
        rows[flag] = {q: store.chunk_results[h.pipeline_id, q] for q in QIDS}
        assert (h.pipeline_id, "q_noemb") not in store.chunk_results
    assert rows[None] == rows[False] and all(len(r) == 3 for r in rows[None].values())
