"""CPU: the grouped merge's numpy restatement (tests/groups_ref.py) on hand-written cases, the host merge of sharded.py
against it, and the question-decomposition pipeline's pure steps against the reference's outputs
(tests/golden/decomposition_golden.json, written by tests/golden/make_golden_decomposition.py)."""

import ast
import json
from pathlib import Path

import numpy as np
import pytest

import groups_ref
from groups_ref import same

GOLDEN = Path(__file__).resolve().parent / "golden"
NAN = float("nan")


# ---- the reference itself, by hand -----------------------------------------------------------------------------------------

def test_ref_order_key_is_the_librarys():
    v = np.array([-np.inf, -1.5, -0.0, 0.0, 5e-324, 1.0, np.inf, np.nan, -np.nan])
    key = groups_ref.dist_to_key(v)
    assert (np.diff(key[:7].astype(object)) > 0).all()          # -inf < -1.5 < -0.0 < +0.0 < denormal < 1 < inf
    assert key[7] == key[8] == groups_ref.KEY_NAN and key[6] < key[7]
    assert int(key[3]) == 0x8000000000000000 and int(key[2]) == 0x7FFFFFFFFFFFFFFF


def test_ref_hand_written_cases():
    vals = [[0.5, 0.1, 0.9], [0.2, 0.1, 0.3], [0.7, 0.0, 0.0]]
    rows = [[7, 3, 9], [7, 5, 3], [1, -1, 9]]
    v, r, c = groups_ref.merge_groups(vals, rows, [0, 2, 3], 4)
    # group 0: row 7 at min(0.5, 0.2), row 3 at min(0.1, 0.3), rows 5 and 9 once; (0.1, 3) before (0.1, 5)
    assert r.tolist() == [[3, 5, 7, 9], [9, 1, -1, -1]] and c.tolist() == [4, 2]
    assert v[0].tolist() == [0.1, 0.1, 0.2, 0.9] and v[1, :2].tolist() == [0.0, 0.7] and np.isnan(v[1, 2:]).all()
    # the cut: count still tells the whole union
    v, r, c = groups_ref.merge_groups(vals, rows, [0, 2, 3], 2)
    assert r.tolist() == [[3, 5], [9, 1]] and c.tolist() == [4, 2]
    # a NaN loses against a number of the same row and stays where it is all a row has; an empty group; G = 0
    v, r, c = groups_ref.merge_groups([[NAN, NAN, 0.5], [0.25, NAN, NAN]], [[3, 5, 9], [3, 5, -4]], [0, 0, 2], 4)
    assert r.tolist() == [[-1] * 4, [3, 9, 5, -1]] and c.tolist() == [0, 3] and np.isnan(v[0]).all()
    assert v[1, :2].tolist() == [0.25, 0.5] and np.isnan(v[1, 2:]).all()
    v, r, c = groups_ref.merge_groups(np.empty((0, 3)), np.empty((0, 3), dtype=np.int64), [0], 2)
    assert v.shape == (0, 2) and r.shape == (0, 2) and c.shape == (0,)
    # signed zeros are two values; rows beyond 2^33 stay apart
    v, r, c = groups_ref.merge_groups([[0.0, -0.0, 0.0, -0.0]], [[1, 2, (1 << 33) + 1, 1]], [0, 1], 3)
    assert r.tolist() == [[1, 2, (1 << 33) + 1]] and np.signbit(v[0]).tolist() == [True, True, False]


# ---- the host merge of the sharded searcher --------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_merge_groups_host_equals_the_reference(seed):
    from autorag_research_amd.sharded import merge_groups_host

    rng = np.random.default_rng(seed)
    S, width = 23, 1 + 6 * seed
    vals = rng.standard_normal((S, width)).round(1)              # coarse values: many ties between rows
    rows = rng.integers(0, 12, (S, width)).astype(np.int64) * ((1 << 33) + 1 if seed == 3 else 1)
    rows[rng.random((S, width)) < 0.15] = -1
    vals[rng.random((S, width)) < 0.15] = np.nan
    vals[rng.random((S, width)) < 0.1] = -np.nan                 # another NaN: one key all the same, rows decide
    vals[0, 0], rows[0, 0], rows[-1, -1] = -np.nan, 11, 11       # (a row that may hold NaNs of both signs alone)
    vals[rng.random((S, width)) < 0.1] = -0.0
    vals[rng.random((S, width)) < 0.1] = 0.0
    sizes = []
    while sum(sizes) < S:
        sizes.append(min(int(rng.integers(0, 6)), S - sum(sizes)))   # ragged, empty groups included
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for k in (1, 5, 40):
        same(merge_groups_host(vals, rows, offs, k), groups_ref.merge_groups(vals, rows, offs, k))


# ---- the pipeline's pure steps against the reference's -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLDEN / "decomposition_golden.json").read_text())


def test_prompt_and_parse_cases(gold):
    from autorag_research_amd.decompose import DEFAULT_DECOMPOSITION_PROMPT, parse_subquestions

    assert DEFAULT_DECOMPOSITION_PROMPT == gold["prompt_template"]
    assert set(gold["parse"]) >= {"numbered_inline", "bullets_inline", "several_question_marks", "empty", "lines"}
    for name, case in gold["parse"].items():
        assert parse_subquestions(case["text"]) == case["subquestions"], name
    assert gold["parse"]["empty"]["subquestions"] == [] and len(gold["parse"]["numbered_inline"]["subquestions"]) == 3


def test_dedupe_against_the_query_and_the_cap(gold):
    from autorag_research_amd.decompose import deduplicate_subquestions

    for case in gold["dedupe"]:
        assert deduplicate_subquestions(case["query"], case["subquestions"], gold["max_subquestions"]) == case["unique"]
    assert len(gold["dedupe"][0]["unique"]) == gold["max_subquestions"]
    for case in gold["dedupe_caps"]:   # the cap is looked at after one was taken: 0 still gives one
        assert deduplicate_subquestions(case["query"], case["subquestions"], case["max_subquestions"]) == case["unique"]
    assert [len(case["unique"]) for case in gold["dedupe_caps"]] == [1, 1, 2, 4]


def test_merge_results_and_scores(gold):
    from autorag_research_amd.decompose import merge_results, normalize_score

    for case in gold["merge"]:
        got = merge_results(case["result_sets"])
        assert got == case["merged"]
        assert [(type(r["doc_id"]), type(r["score"]), list(r)) for r in got] == \
               [(type(r["doc_id"]), type(r["score"]), list(r)) for r in case["merged"]]   # 1 == 1.0 == True; key order
        assert all(r is not s for r in got for rs in case["result_sets"] for s in rs)          # copies
    assert [r["doc_id"] for r in gold["merge"][1]["merged"]] == [1, 10, 2]     # '1' < '10' < '2'
    for text, want in gold["normalize_score"]:
        got = normalize_score(ast.literal_eval(text))   # reprs of 1, 0.25, True, None, '0.5', ...
        assert type(got) is float and got == want, text


def test_config_dict(gold):
    from autorag_research_amd.decompose import (
        Mi355QuestionDecompositionPipelineConfig,
        Mi355QuestionDecompositionRetrievalPipeline,
    )

    class Inner:
        retrieval_unit = "chunk"
        pipeline_id = gold["inner_pipeline_id"]

    class Reranker:
        model_name = "fake-reranker"

    for key, reranker in (("config", None), ("config_reranked", Reranker())):
        p = Mi355QuestionDecompositionRetrievalPipeline.__new__(Mi355QuestionDecompositionRetrievalPipeline)
        p._inner_retrieval_pipeline, p._reranker = Inner(), reranker
        p._decomposition_prompt_template = gold["prompt_template"]
        p.max_subquestions, p.fetch_k_multiplier = gold["max_subquestions"], gold["fetch_k_multiplier"]
        assert p._get_pipeline_config() == {**gold[key], "type": "mi355_question_decomposition"}
    cfg = Mi355QuestionDecompositionPipelineConfig(name="qd", llm=object(), inner_retrieval_pipeline_name="vs")
    assert (cfg.max_subquestions, cfg.fetch_k_multiplier, cfg.reranker) == (3, 2, None)
    assert cfg.get_pipeline_kwargs()["inner_retrieval_pipeline"] == "vs"
    inner = Inner()
    cfg.inject_retrieval_pipeline(inner)
    assert cfg.get_pipeline_kwargs()["inner_retrieval_pipeline"] is inner
    assert cfg.get_pipeline_class() is Mi355QuestionDecompositionRetrievalPipeline
