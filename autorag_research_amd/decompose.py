"""Question-decomposition retrieval on the MI355X path.

Mirrors the reference's QuestionDecompositionRetrievalPipelineConfig / QuestionDecompositionRetrievalPipeline
(pipelines/retrieval/question_decomposition.py:56-294): an LLM splits the question into up to `max_subquestions`
sub-questions, the inner retrieval pipeline answers the question and every sub-question at `top_k * fetch_k_multiplier`, the
lists are merged by "every chunk once, at its best score" (`_merge_results`, :203-220) and optionally reranked (:239-259).

What this module adds: when the inner pipeline is one of this package's vector-search pipelines, the sub-queries of a
question -- and, in `run()`, of a whole page of questions -- are searched and merged in ONE grouped call on the GPU
(Mi355RetrievalService.vector_search_groups -> mi355dr_search_groups), instead of one search per sub-question and a loop
over dicts per question.  Any other inner pipeline (hybrid, the reference's BM25, ...) takes the reference's flow over its
retrieval-pipeline surface and the host `_merge_results`; so does a shape beyond the grouped call's caps: lists longer than
1024 (`top_k * fetch_k_multiplier`), or more than 4096 entries in the lists of one question
(`(1 + max_subquestions) * top_k * fetch_k_multiplier`).

The parse / dedupe / merge / rerank steps are written from the reference's behaviour, which
tests/golden/decomposition_golden.json records; only the prompt template is its text.

Documented difference (device path only): the grouped call cuts each question's union at the number of results asked for by
(distance, index row); the reference sorts the whole union by (-score, str(doc_id)) and then cuts.  The two agree unless an
exact score tie straddles the cut; inside the returned list the reference's order is restored.
"""

from __future__ import annotations

import asyncio
import inspect
import itertools
import logging
import re
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any

from .compat import BaseRetrievalPipelineConfig
from .gqr import _load_child
from .pipelines import Mi355BaseRetrievalPipeline, _VectorSearchMixin, child_page, get_retrieval_pipeline_unit

logger = logging.getLogger("AutoRAG-Research")

TEXT_RETRIEVAL_UNIT = "chunk"
_GROUP_LIST_CAP = 1024      # the grouped call's caps (include/mi355dr.h "grouped search"): the length of one list,
_GROUP_ENTRIES_CAP = 4096   # and the entries of one group, all its lists together

DEFAULT_DECOMPOSITION_PROMPT = """You are decomposing a question for retrieval-augmented generation.

Question: {query}

Write up to {max_subquestions} short, standalone sub-questions that would help retrieve evidence.
Return one sub-question per line and no other text.
If decomposition is unnecessary, repeat the original question once.

Sub-questions:"""  # the reference's template (question_decomposition.py:21-29)

# What may stand in front of a sub-question: a "Question 2:" / "Sub-question:" label, a bullet, "3." / "3)", "b." / "b)".
_BULLETS = "-*\u2022"
_ITEM_MARK = rf"\d+[.)]|[{_BULLETS}]"
_LEAD_RE = re.compile(rf"(?:(?:sub-?)?question\s*\d*\s*:|{_ITEM_MARK}|[a-z][.)])\s*", re.IGNORECASE)
_ITEM_START_RE = re.compile(rf"(?<=\s)(?:{_ITEM_MARK})")   # a list item that begins inside a line
_SENTENCE_END_RE = re.compile(r"\?\s+")                     # a question mark with more text behind it


def normalize_question(question: str) -> str:
    """What two questions are compared by: letter case and the amount of white space do not count."""
    return " ".join(question.split()).lower()


def normalize_score(score: Any) -> float:
    """The score of a result dict as a float; whatever is no int or float (None, a string) counts 0.0, a bool as 0 / 1."""
    if not isinstance(score, (int, float)):
        return 0.0
    return float(score)


def _cut(line: str, cuts: list[int]) -> list[str]:
    """`line` cut at the positions `cuts`: the pieces without their outer white space, empty ones left out."""
    edges = [0, *cuts, len(line)]
    pieces = (line[lo:hi].strip() for lo, hi in zip(edges, edges[1:]))
    return [piece for piece in pieces if piece]


def parse_subquestions(decomposition_text: str) -> list[str]:
    """The LLM's answer -> sub-questions, with the reference's outputs (tests/golden/decomposition_golden.json pins them).
    Several lines: one sub-question per non-empty line.  One line: cut in front of every numbered or bulleted item that
    follows white space; if there is none and the line holds more than one '?', cut behind every '?' that white space
    follows.  Each piece then loses one leading label / bullet / number / letter, its outer white space and at last any
    trailing blanks and semicolons; pieces of which nothing is left are dropped."""
    pieces = [line for line in map(str.strip, decomposition_text.splitlines()) if line]
    if len(pieces) == 1:
        (line,) = pieces
        starts = [m.start() for m in _ITEM_START_RE.finditer(line)]
        if starts:
            pieces = _cut(line, starts)
        elif line.count("?") >= 2:
            pieces = _cut(line, [m.end() for m in _SENTENCE_END_RE.finditer(line)])
    found = []
    for piece in pieces:
        lead = _LEAD_RE.match(piece)
        body = (piece[lead.end():] if lead else piece).strip().rstrip("; ")
        if body:
            found.append(body)
    return found


def deduplicate_subquestions(query: str, subquestions: list[str], max_subquestions: int) -> list[str]:
    """The sub-questions in first-seen order, each once under `normalize_question`, none that is blank or repeats `query`,
    cut at `max_subquestions` -- but never below one: the reference looks at its cap only after it has taken one."""
    first_of: dict[str, str] = {}
    for subquestion in subquestions:
        first_of.setdefault(normalize_question(subquestion), subquestion)
    for not_wanted in ("", normalize_question(query)):
        first_of.pop(not_wanted, None)
    return list(first_of.values())[: max(max_subquestions, 1)]


def merge_results(result_sets: list[list[dict[str, Any]]]) -> list[dict[str, Any]]:
    """The lists of one question fused: every doc_id once, as a copy of the dict that brought its highest score (of equal
    scores the earliest) with that score as a float, ordered by falling score and, between equal scores, by str(doc_id);
    doc ids that compare equal as strings keep the order in which they first appeared.  Results without a doc_id are
    ignored."""
    best: dict[Any, tuple[float, dict[str, Any]]] = {}   # doc_id -> (score, result), in order of first appearance
    for result in itertools.chain.from_iterable(result_sets):
        doc_id = result.get("doc_id")
        if doc_id is None:
            continue
        score = normalize_score(result.get("score"))
        if doc_id not in best or best[doc_id][0] < score:
            best[doc_id] = (score, dict(result, score=score))
    ranked = sorted(best.values(), key=lambda entry: (-entry[0], str(entry[1]["doc_id"])))
    return [result for _, result in ranked]


@dataclass(kw_only=True)
class Mi355QuestionDecompositionPipelineConfig(BaseRetrievalPipelineConfig):
    """Fields as QuestionDecompositionRetrievalPipelineConfig (:56-97) + `device`.  The inner pipeline is injected
    (`inject_retrieval_pipeline`, as the reference's Executor does) or, failing that, loaded by its name."""

    llm: Any
    inner_retrieval_pipeline_name: str
    reranker: Any | None = None
    decomposition_prompt_template: str = field(default=DEFAULT_DECOMPOSITION_PROMPT)
    max_subquestions: int = 3
    fetch_k_multiplier: int = 2
    device: int = 0
    _inner_retrieval_pipeline: Any | None = field(default=None, repr=False)

    def __setattr__(self, name: str, value: Any) -> None:
        if name in ("llm", "reranker") and isinstance(value, str):
            try:
                from autorag_research import injection  # type: ignore
            except Exception as e:  # noqa: BLE001
                raise ValueError(f"{name} {value!r} was given by name, which needs autorag_research.injection; "  # noqa: TRY003
                                 "pass an instance instead") from e
            value = injection.load_llm(value) if name == "llm" else injection.load_reranker(value)
        super().__setattr__(name, value)

    def get_pipeline_class(self) -> type["Mi355QuestionDecompositionRetrievalPipeline"]:
        return Mi355QuestionDecompositionRetrievalPipeline

    def get_pipeline_kwargs(self) -> dict[str, Any]:
        return {"llm": self.llm,
                "inner_retrieval_pipeline": self._inner_retrieval_pipeline or self.inner_retrieval_pipeline_name,
                "reranker": self.reranker, "decomposition_prompt_template": self.decomposition_prompt_template,
                "max_subquestions": self.max_subquestions, "fetch_k_multiplier": self.fetch_k_multiplier,
                "device": self.device}

    def inject_retrieval_pipeline(self, pipeline: Any) -> None:
        self._inner_retrieval_pipeline = pipeline


class Mi355QuestionDecompositionRetrievalPipeline(Mi355BaseRetrievalPipeline):
    """Decompose the question, retrieve for every part, merge, optionally rerank; the vector-search case on the GPU."""

    def __init__(self, session_factory: Any, name: str, llm: Any, inner_retrieval_pipeline: Any, reranker: Any | None = None,
                 decomposition_prompt_template: str = DEFAULT_DECOMPOSITION_PROMPT, max_subquestions: int = 3,
                 fetch_k_multiplier: int = 2, schema: Any | None = None, config_dir: Path | None = None, device: int = 0):
        if isinstance(inner_retrieval_pipeline, str):
            inner_retrieval_pipeline = _load_child(inner_retrieval_pipeline, session_factory, schema, config_dir)
        self._llm = llm
        self._inner_retrieval_pipeline = inner_retrieval_pipeline
        self._decomposition_prompt_template = decomposition_prompt_template
        self.max_subquestions = max_subquestions
        self.fetch_k_multiplier = fetch_k_multiplier
        self._reranker = reranker
        if reranker is not None and self.retrieval_unit != TEXT_RETRIEVAL_UNIT:  # (:37-53)
            raise ValueError("Question decomposition reranking requires a text chunk retrieval pipeline "  # noqa: TRY003
                             f"(retrieval_unit='chunk'); got retrieval_unit={self.retrieval_unit!r} from "
                             f"{type(inner_retrieval_pipeline).__name__!r}.")
        super().__init__(session_factory, name, schema, device=device)

    @property
    def retrieval_unit(self):  # type: ignore[override]
        return get_retrieval_pipeline_unit(self._inner_retrieval_pipeline)

    def _get_pipeline_config(self) -> dict[str, Any]:
        return {"type": "mi355_question_decomposition", "retrieval_unit": self.retrieval_unit,
                "max_subquestions": self.max_subquestions, "fetch_k_multiplier": self.fetch_k_multiplier,
                "decomposition_prompt_template": self._decomposition_prompt_template,
                "inner_retrieval_pipeline_id": getattr(self._inner_retrieval_pipeline, "pipeline_id", None),
                "reranker_model": self._reranker.model_name if self._reranker is not None else None}

    # ---- the reference's pure steps, under its names ----
    _normalize_question = staticmethod(normalize_question)
    _normalize_score = staticmethod(normalize_score)
    _parse_subquestions = staticmethod(parse_subquestions)
    _merge_results = staticmethod(merge_results)

    def _deduplicate_subquestions(self, query: str, subquestions: list[str]) -> list[str]:
        return deduplicate_subquestions(query, subquestions, self.max_subquestions)

    def _build_decomposition_prompt(self, query: str) -> str:
        return self._decomposition_prompt_template.format(query=query, max_subquestions=self.max_subquestions)

    async def _decompose(self, query_text: str) -> list[str]:
        prompt = self._build_decomposition_prompt(query_text)
        if hasattr(self._llm, "ainvoke"):
            response = await self._llm.ainvoke(prompt)
        else:
            response = self._llm(prompt)
            if inspect.isawaitable(response):
                response = await response
        text = response.content if hasattr(response, "content") else str(response)
        return self._deduplicate_subquestions(query_text, self._parse_subquestions(text))

    # ---- rerank: what the reference's :222-259 do ----
    def _chunk_unit(self):
        """The exported chunk table with its index.  An inner pipeline of this package already holds one in its service;
        the wrapper's own service exports the table only where the inner pipeline is somebody else's."""
        inner_service = getattr(self._inner_retrieval_pipeline, "_service", None)
        service = inner_service if hasattr(inner_service, "_unit") else self._service
        return service._unit(TEXT_RETRIEVAL_UNIT)

    def _load_contents_for_results(self, results: list[dict[str, Any]]) -> list[dict[str, Any]]:
        """The results, those without a text (None or "") completed from the chunk table; "" where the table has none."""
        if all(r.get("content") not in (None, "") for r in results):
            return results
        u = self._chunk_unit()
        pos, contents = u.pos_of_id(), u.table.contents
        return [r if r.get("content") not in (None, "")
                else {**r, "content": (contents[pos[r["doc_id"]]] or "") if r["doc_id"] in pos else ""} for r in results]

    async def _rerank_results(self, query_text: str, merged: list[dict[str, Any]], top_k: int) -> list[dict[str, Any]]:
        """The reranker's top_k over every merged result that has a text, as {doc_id, score, content} with the reranker's
        score.  Without a reranker, and where no result has a text, the head of the merged list stands."""
        pool = []
        if self._reranker is not None:
            pool = [r for r in self._load_contents_for_results(merged) if r.get("content")]
        if not pool:
            return merged[:top_k]
        hits = await self._reranker.arerank(query_text, [str(r["content"]) for r in pool], top_k=top_k)
        return [dict(doc_id=pool[hit.index]["doc_id"], score=hit.score, content=pool[hit.index]["content"]) for hit in hits]

    # ---- which path ----
    def _device_path(self, top_k: int) -> bool:
        """The inner pipeline is one of this package's vector-search pipelines and the question's lists fit the grouped call
        (include/mi355dr.h "grouped search"): each list at most 1024 long, and the lists of one question -- the question and
        its sub-questions, `top_k * fetch_k_multiplier` each -- at most 4096 entries when rounded up to a power of two.
        Larger shapes take the generic path, which has no such cap.
        Not the text pipeline in multi mode: like the reference's, it answers a TEXT with a single-vector search
        (vector_search.py:171-191), so the lists of one question would come from two indexes -- the generic path serves it."""
        inner = self._inner_retrieval_pipeline
        if not isinstance(inner, _VectorSearchMixin) or (inner.search_mode == "multi" and inner.retrieval_unit != "image_chunk"):
            return False
        fetch_k = top_k * self.fetch_k_multiplier
        entries = (1 + max(self.max_subquestions, 1)) * fetch_k   # (`deduplicate_subquestions` keeps at least one)
        return 1 <= fetch_k <= _GROUP_LIST_CAP and entries <= _GROUP_ENTRIES_CAP

    def _union_k(self, top_k: int, n_lists: int) -> int:
        """What the grouped call is asked for: top_k, or -- a reranker sees every candidate -- the whole union."""
        return top_k if self._reranker is None else max(1, n_lists) * top_k * self.fetch_k_multiplier

    def _query_text(self, query_id) -> str | None:
        q = self._service.get_queries([query_id])[0]
        return None if q is None else q.contents

    def _stored_embedding(self, row: Any, what: Any):
        inner = self._inner_retrieval_pipeline
        emb = None if row is None else (row.embeddings if inner.search_mode == "multi" else row.embedding)
        if emb is None:
            raise ValueError(f"Query {what} has no stored embedding for search_mode={inner.search_mode!r}")  # noqa: TRY003
        return emb

    async def _embed_texts(self, texts: list[str], lookup: bool = True, strict: bool = True) -> list:
        """Embeddings of sub-questions as the inner pipeline's `retrieve()` resolves them: a stored query with that exact
        text answers with its stored embedding, any other text goes to the inner pipeline's embedding model (rank 0).
        `lookup=False`: every text goes to the model, as `_retrieve_by_text` does.
        `strict=False` (the page form): a text that cannot be embedded -- a stored query without an embedding, or one the
        model fails on when the batch is asked again text by text -- is logged and answered with None, not raised."""
        inner = self._inner_retrieval_pipeline
        out: list[Any] = [None] * len(texts)
        fresh = []
        for i, t in enumerate(texts):
            stored = inner._service.find_query_by_text(t) if lookup else None
            if stored is None:
                fresh.append(i)
                continue
            try:
                out[i] = self._stored_embedding(stored, stored.id)
            except ValueError:
                if strict:
                    raise
                logger.error(f"sub-question {t!r} is stored query {stored.id}, which has no embedding")
        if fresh:
            model = inner._embedding_model
            if model is None:
                from .compat import EmbeddingError  # noqa: PLC0415

                raise EmbeddingError
            batched = hasattr(model, "embed_queries")   # query-side embeddings (hyde.py explains why not embed_documents)

            async def embed_batch(batch: list[str]) -> list:
                if batched:
                    return list(model.embed_queries(batch))
                return await asyncio.gather(*[model.aembed_query(t) for t in batch])

            async def embed():
                batch = [texts[i] for i in fresh]
                try:
                    return await embed_batch(batch)
                except Exception:  # noqa: BLE001
                    if strict:
                        raise
                    logger.exception("embedding the page's sub-questions failed; asking text by text")
                alone = []
                for t in batch:
                    try:
                        alone.append((await embed_batch([t]))[0])
                    except Exception:  # noqa: BLE001 - the question of that text alone is reported as failed
                        logger.exception(f"no embedding for sub-question {t!r}")
                        alone.append(None)
                return alone

            for i, v in zip(fresh, await self._service.on_root(embed)):
                out[i] = v
        return out

    def _search_groups(self, groups: list[list], top_ks: list[int], fetch_k: int) -> list[list[dict]]:
        """ONE grouped call for all questions; each is cut at its own number of results afterwards."""
        inner = self._inner_retrieval_pipeline
        block = inner._service.vector_search_groups(groups, max(top_ks), fetch_k, unit=inner.retrieval_unit or "chunk",
                                                    search_mode=inner.search_mode)
        return [res[:k] for res, k in zip(block, top_ks)]

    # ---- per query (:261-294) ----
    async def _retrieve(self, query_text: str, first: Any, by_id: bool, top_k: int) -> list[dict[str, Any]]:
        fetch_k = top_k * self.fetch_k_multiplier
        subquestions = await self._service.on_root(lambda: self._decompose(query_text))
        inner = self._inner_retrieval_pipeline
        if self._device_path(top_k):
            head = self._stored_embedding(self._service.get_queries([first])[0], first) if by_id else None
            embs = await self._embed_texts(subquestions if by_id else [query_text, *subquestions], lookup=by_id)
            group = [head, *embs] if by_id else embs
            merged = self._search_groups([group], [self._union_k(top_k, len(group))], fetch_k)[0]
        else:
            if by_id:
                result_sets = [await inner._retrieve_by_id(first, fetch_k)]
                for sq in subquestions:
                    result_sets.append(await inner.retrieve(sq, fetch_k))
            else:
                result_sets = [await inner._retrieve_by_text(query_text, fetch_k)]
                for sq in subquestions:
                    result_sets.append(await inner._retrieve_by_text(sq, fetch_k))
            merged = self._merge_results(result_sets)
        return await self._rerank_results(query_text, merged, top_k)

    async def _retrieve_by_id(self, query_id, top_k: int) -> list[dict[str, Any]]:
        query_text = self._query_text(query_id)
        if query_text is None:
            raise ValueError(f"Query {query_id} not found")  # noqa: TRY003  (fetch_query_texts, retrieval_pipeline.py:552-571)
        return await self._retrieve(query_text, query_id, True, top_k)

    async def _retrieve_by_text(self, query_text: str, top_k: int) -> list[dict[str, Any]]:
        return await self._retrieve(query_text, None, False, top_k)

    # ---- a page ----
    def _retrieve_block(self, query_ids: list, top_k: int) -> list[list[dict] | None]:
        """A page: all decompositions generated concurrently on rank 0 (HyDE's retry rule, and its ordering of collectives:
        ONE read of the query rows first, ONE broadcast of what rank 0 made), the sub-questions embedded in one batch, the
        whole page searched and merged in ONE grouped call.  A query whose decomposition, stored embedding, sub-question
        embedding or reranking fails is answered None and fails alone; a failure of the grouped call itself is raised, and
        `run()` then asks the page again query by query."""
        fetch_k = top_k * self.fetch_k_multiplier
        rows = self._service.get_queries(list(query_ids))
        inner = self._inner_retrieval_pipeline

        def decompose_page():
            async def page():
                attempts, delay0 = getattr(self, "_run_retry", (1, 0.0))

                async def one(qid, row):
                    delay = delay0
                    for attempt in range(attempts):
                        try:
                            if row is None:
                                raise ValueError(f"Query {qid} not found")  # noqa: TRY003, TRY301
                            return await self._decompose(row.contents)
                        except Exception:  # noqa: BLE001
                            if attempt + 1 >= attempts:
                                logger.exception(f"question decomposition failed for query {qid} after {attempts} attempts")
                                return None
                            await asyncio.sleep(min(max(delay, delay0), 60))
                            delay *= 2
                    return None

                return await asyncio.gather(*[one(q, r) for q, r in zip(query_ids, rows)])

            return asyncio.run(page())

        subs = self._service.from_root(decompose_page)
        out: list[list[dict] | None] = [None] * len(query_ids)
        live = [i for i, s in enumerate(subs) if s is not None]
        if not self._device_path(top_k):
            # the generic path: the inner pipeline's page for the ids, its `retrieve` for the sub-questions, the host merge
            first = child_page(inner, [query_ids[i] for i in live], fetch_k)

            async def rest():
                for i, head in zip(live, first):
                    if head is None:
                        continue
                    try:
                        sets = [head] + [await inner.retrieve(sq, fetch_k) for sq in subs[i]]
                        out[i] = await self._rerank_results(rows[i].contents, self._merge_results(sets), top_k)
                    except Exception:  # noqa: BLE001 - that query alone is reported as failed
                        logger.exception(f"question decomposition retrieval failed for query {query_ids[i]}")

            asyncio.run(rest())
            return out
        heads = {}
        for i in live:
            try:
                heads[i] = self._stored_embedding(rows[i], query_ids[i])
            except ValueError:
                logger.error(f"Retrieval failed for query {query_ids[i]}")
        live = [i for i in live if i in heads]
        if not live:
            return out
        flat = [sq for i in live for sq in subs[i]]
        embs = iter(asyncio.run(self._embed_texts(flat, strict=False)) if flat else [])
        groups = {i: [heads[i], *[next(embs) for _ in subs[i]]] for i in live}
        live = [i for i in live if all(e is not None for e in groups[i])]   # (the failures are logged where they happen)
        if not live:
            return out
        page = self._search_groups([groups[i] for i in live], [self._union_k(top_k, len(groups[i])) for i in live], fetch_k)

        async def rerank_page():
            for i, merged in zip(live, page):
                try:
                    out[i] = await self._rerank_results(rows[i].contents, merged, top_k)
                except Exception:  # noqa: BLE001 - that query alone is reported as failed
                    logger.exception(f"question decomposition reranking failed for query {query_ids[i]}")

        asyncio.run(rerank_page())
        return out


__all__ = ["DEFAULT_DECOMPOSITION_PROMPT", "Mi355QuestionDecompositionPipelineConfig",
           "Mi355QuestionDecompositionRetrievalPipeline", "deduplicate_subquestions", "merge_results", "normalize_score",
           "parse_subquestions"]
