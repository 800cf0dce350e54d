"""Writes tests/golden/decomposition_golden.json from the reference's QuestionDecompositionRetrievalPipeline
(pipelines/retrieval/question_decomposition.py), build container only -- the tests read the file and never import the
reference.  Run:  python tests/golden/make_golden_decomposition.py

Contents:
  parse / dedupe / merge / config   the pipeline's pure steps on hand-written inputs (numbered inline, bullets, several '?'
                                    on one line, empty text; repeats of the question and the cap; the '1' < '10' < '2' string
                                    order between equal scores; the persisted config dict), and the corners a restatement of
                                    these steps can get wrong (what counts as white space, a digit, a letter or a line break;
                                    the cap looked at after one was taken; doc ids that are equal as keys or as strings).
  flows                             `_retrieve_by_id` / `_retrieve_by_text` over the fake Unit of Work of make_golden.py with
                                    the reference's VectorSearchRetrievalPipeline (single mode) as the inner pipeline, a fake
                                    LLM that answers a fixed multi-line decomposition and the stand-in embedding of
                                    `hyde_fake_models`; one flow with a fake reranker, with the documents it was handed.
No recorded flow has two equal scores across its cut at top_k (asserted below): the device path cuts by (distance, row), the
reference by (-score, str(doc_id)), and a fixture must not depend on which.
"""

from __future__ import annotations

import asyncio
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402  (imports the reference through ref_import.import_reference)

from autorag_research.pipelines.retrieval.question_decomposition import (  # noqa: E402
    DEFAULT_DECOMPOSITION_PROMPT,
    QuestionDecompositionRetrievalPipeline,
)
from autorag_research.pipelines.retrieval.vector_search import VectorSearchRetrievalPipeline  # noqa: E402

DECOMPOSITION = ("1. query text 3\n"            # a stored query: answered from its stored embedding
                 "2) What is late interaction?\n"
                 "- {query}\n"                   # the question itself: dropped
                 "* how are chunks scored ;\n"
                 "Sub-question 4: one too many")  # beyond max_subquestions = 3

PARSE_CASES = {
    "lines": DECOMPOSITION.replace("{query}", "query text 0"),
    "numbered_inline": "1. Who wrote it? 2. When was it published? 3) Where",
    "bullets_inline": "- first part - second part • third part",
    "several_question_marks": "Who wrote it? When was it published?  Why?",
    "one_line": "Just one question",
    "prefixes": "Question 2: what now\nsub-question: and then ;\na) lettered\nB. Lettered too",
    "empty": "   \n ",
    # what a rewrite of these steps could get wrong
    "marks_need_white_space_in_front": "v1.2) stays whole, a-b too",
    "inline_runs_of_white_space": "first \t 1) second   -  third\u00a0\u2022 fourth 12.fifth",
    "numbered_wins_over_question_marks": "Who? Why? 2. When?",
    "question_mark_without_white_space_behind": "a?b c? d? e?",
    "question_marks_in_a_row": "what??  really? ?",
    "only_the_first_prefix_goes": "1. 2. - nested",
    "labels": "QUESTION12 : upper\nSubquestion 3:tight\nsub-question4:x\nQuestions: not a label\nquestion 2 no colon",
    "letters": "a) one\nZ. two\nab) not a letter prefix\n\u017f) long s\n\u212a. kelvin",
    "other_digits": "\u0663) arabic-indic three\n\u00b2) superscript two",
    "nothing_left": "- \n* ;\n3. ; ;\n?",
    "trailing": "keep inner ; this ; ; \nx ;\t\ny\t;\nz;;  ;",
    "line_breaks": "one\r\ntwo\x0bthree\x0cfour\u2028five\x85six",
    "one_line_of_several_blank_ones": "\n\n  - only - this  \n\n",
}

DEDUPE_CASES = [
    {"query": "What is  MaxSim?", "subquestions": ["what is maxsim?", "How is it computed?", "HOW is it   computed?", "  ",
                                                  "Why late interaction?", "Which models?", "One more?"]},
    {"query": "q", "subquestions": []},
    {"query": "  ", "subquestions": ["", "A  b", "a B", "\tc\n", "C", "STRASSE", "stra\u00dfe", "\u0130x", "i\u0307x", "d", "e"]},
    {"query": "Q\u00a0one", "subquestions": ["q one", "q\u3000ONE", "two", "q  one", "two ", "three"]},
]

MERGE_CASES = [
    [[{"doc_id": 2, "score": 0.5, "content": "two"}, {"doc_id": 10, "score": 0.5}, {"doc_id": 1, "score": 0.5}],
     [{"doc_id": 1, "score": 0.75, "content": "one"}, {"doc_id": None, "score": 9.0}, {"doc_id": 3, "score": "bad"},
      {"doc_id": 10, "score": 0.5, "content": "later, not better"}],
     [{"doc_id": 4, "score": None}, {"doc_id": 2, "score": 0.25}, {"doc_id": "7", "score": 1}]],
    [[{"doc_id": 1, "score": 0.5}, {"doc_id": 10, "score": 0.5}, {"doc_id": 2, "score": 0.5}]],
    [],
    [[], [{"doc_id": "a"}], []],                                                  # no score at all
    [[{"doc_id": 5, "score": True, "content": "bool"}, {"doc_id": 6, "score": 1}, {"doc_id": 5, "score": 1.0, "content": "equal"}],
     [{"doc_id": 6, "score": 2, "extra": [1]}, {"score": 3.0}, {"doc_id": 0, "score": -0.0}, {"doc_id": "0", "score": 0}]],
    [[{"doc_id": 1, "score": 0.5, "content": "int"}], [{"doc_id": "1", "score": 0.5, "content": "str"}],
     [{"doc_id": 1.0, "score": 0.75, "content": "float, the same key as the int"}]],
    [[{"content": "key order", "score": 1, "doc_id": 9}, {"doc_id": 8, "content": "no score key"}],
     [{"doc_id": 9, "score": 0.5, "content": "worse"}, {"doc_id": -3, "score": -1.5}, {"doc_id": 8, "score": -2}]],
]


class _Queries(mg._FakeQueryRepo):
    def find_by_contents(self, text):
        return next((q for q in self.queries.values() if getattr(q, "contents", None) == text), None)


class FakeLLM:
    async def ainvoke(self, prompt):
        return mg._Obj(content=DECOMPOSITION.replace("{query}", prompt.split("Question: ")[1].split("\n")[0]))


class FakeReranker:
    """Scores a document by its bytes; remembers what it was handed."""

    model_name = "fake-reranker"

    def __init__(self):
        self.seen = []

    @staticmethod
    def score(text):
        return (sum((i + 1) * b for i, b in enumerate(text.encode())) % 997) / 997.0

    async def arerank(self, query, documents, top_k=None):
        self.seen.append(list(documents))
        ranked = sorted((mg._Obj(index=i, text=d, score=self.score(d)) for i, d in enumerate(documents)),
                        key=lambda r: r.score, reverse=True)
        return ranked[:top_k]


def _pipeline(svc, inner, reranker=None):
    p = QuestionDecompositionRetrievalPipeline.__new__(QuestionDecompositionRetrievalPipeline)
    p._llm, p._inner_retrieval_pipeline, p._reranker, p._service = FakeLLM(), inner, reranker, svc
    p._decomposition_prompt_template, p.max_subquestions, p.fetch_k_multiplier = DEFAULT_DECOMPOSITION_PROMPT, 3, 2
    return p


def main() -> None:
    mg.make_service()
    svc = mg._LAST["svc"]
    svc._uow.queries = _Queries(svc._uow.queries.queries)
    _, emb = mg.hyde_fake_models(32)
    inner = VectorSearchRetrievalPipeline.__new__(VectorSearchRetrievalPipeline)
    inner.search_mode, inner._service, inner._embedding_model, inner.pipeline_id = "single", svc, emb, 41
    p = _pipeline(svc, inner)

    out = {"prompt_template": DEFAULT_DECOMPOSITION_PROMPT, "decomposition": DECOMPOSITION, "max_subquestions": 3,
           "fetch_k_multiplier": 2, "inner_pipeline_id": 41}
    out["parse"] = {name: {"text": text, "subquestions": p._parse_subquestions(text)} for name, text in PARSE_CASES.items()}
    out["dedupe"] = [{**c, "unique": p._deduplicate_subquestions(c["query"], c["subquestions"])} for c in DEDUPE_CASES]
    out["dedupe_caps"] = []
    for cap in (0, 1, 2, 9):   # the cap is looked at after one was taken: 0 still gives one
        capped = _pipeline(svc, inner)
        capped.max_subquestions = cap
        out["dedupe_caps"].append({**DEDUPE_CASES[0], "max_subquestions": cap,
                                   "unique": capped._deduplicate_subquestions(DEDUPE_CASES[0]["query"], DEDUPE_CASES[0]["subquestions"])})
    out["merge"] = [{"result_sets": sets, "merged": p._merge_results(sets)} for sets in MERGE_CASES]
    out["normalize_score"] = [[repr(v), p._normalize_score(v)] for v in (1, 0.25, True, None, "0.5", -3, False, [1.5], 1e300)]
    out["config"] = p._get_pipeline_config()
    rr = FakeReranker()
    out["config_reranked"] = _pipeline(svc, inner, rr)._get_pipeline_config()

    loop = asyncio.new_event_loop()

    def flow(pipe, top_k, query_id=None, text=None):
        unions = []
        merge = pipe._merge_results
        pipe._merge_results = lambda sets: unions.append(merge(sets)) or unions[-1]
        call = pipe._retrieve_by_id(query_id, top_k) if query_id is not None else pipe._retrieve_by_text(text, top_k)
        results = loop.run_until_complete(call)
        del pipe._merge_results
        union = unions[0]
        if pipe._reranker is None and len(union) > top_k:  # the documented difference must not decide a fixture
            assert union[top_k - 1]["score"] != union[top_k]["score"], (query_id, text)
        return {"top_k": top_k, "results": results, "union_ids": [r["doc_id"] for r in union]}

    out["by_id"] = {q: flow(p, 5, query_id=q) for q in ("q0", "q2", "q3", "q5")}
    out["by_id_k1"] = {"q4": flow(p, 1, query_id="q4")}
    out["by_text"] = {"text": "what is late interaction?", **flow(p, 5, text="what is late interaction?")}
    pr = _pipeline(svc, inner, rr)
    out["reranked"] = {"q1": flow(pr, 4, query_id="q1")}
    out["reranked"]["q1"]["documents"] = rr.seen[0]
    loop.close()
    (HERE / "decomposition_golden.json").write_text(json.dumps(out, indent=1))
    print("wrote decomposition_golden.json")


if __name__ == "__main__":
    main()
