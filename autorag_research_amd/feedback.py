"""Vector search with Rocchio pseudo-relevance feedback on the MI355X path.

The classical no-LLM counterpart of the query-expansion pipelines of this package (HyDE, question decomposition, GQR):
every query is searched at `fb_k`, moved towards the mean of its own first results -- alpha * query + beta * mean, terms
unit-normalised (Rocchio 1971, without negatives) -- and searched again at `top_k`.  Both passes and the combination run
on the GPU in one library call per page (`mi355dr_search_feedback`): the first pass's lists and the chunks' vectors never
reach the host.  This pipeline is `Mi355VectorSearchRetrievalPipeline` in single mode with its searches answered by
`Mi355RetrievalService.vector_search_feedback`.  One feedback round; not under a process group (the service raises).
"""

from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Any

from .compat import BaseRetrievalPipelineConfig, EmbeddingError
from .pipelines import Mi355BaseRetrievalPipeline

logger = logging.getLogger("AutoRAG-Research")


@dataclass(kw_only=True)
class Mi355FeedbackPipelineConfig(BaseRetrievalPipelineConfig):
    """Fields of Mi355VectorSearchPipelineConfig without `search_mode` (single vectors only) + the feedback's depth and
    weights."""

    embedding_model: Any | str | None = None
    fb_k: int = 10
    alpha: float = 1.0
    beta: float = 0.75
    device: int = 0

    def __setattr__(self, name: str, value: Any) -> None:
        if name == "embedding_model" and isinstance(value, str):
            from .embeddings import load_embedding_model

            value = load_embedding_model(value)
        super().__setattr__(name, value)

    def get_pipeline_class(self) -> type["Mi355FeedbackRetrievalPipeline"]:
        return Mi355FeedbackRetrievalPipeline

    def get_pipeline_kwargs(self) -> dict[str, Any]:
        return {"embedding_model": self.embedding_model, "fb_k": self.fb_k, "alpha": self.alpha, "beta": self.beta,
                "device": self.device}


class Mi355FeedbackRetrievalPipeline(Mi355BaseRetrievalPipeline):
    """Search at fb_k -> query + mean of its results -> search at top_k, over `chunk` rows on the GPU."""

    retrieval_unit = "chunk"

    def __init__(self, session_factory: Any, name: str, embedding_model: Any | None = None, fb_k: int = 10,
                 alpha: float = 1.0, beta: float = 0.75, schema: Any | None = None, device: int = 0):
        if not 1 <= int(fb_k) <= 1024:
            raise ValueError("fb_k must lie in [1, 1024]")
        if not (0.0 <= float(alpha) < float("inf") and 0.0 <= float(beta) < float("inf")):
            raise ValueError("alpha and beta must be finite and >= 0")
        # set BEFORE super().__init__: _get_pipeline_config() is called there
        self._embedding_model = embedding_model
        self.fb_k, self.alpha, self.beta = int(fb_k), float(alpha), float(beta)
        super().__init__(session_factory, name, schema, device=device)

    def _get_pipeline_config(self) -> dict[str, Any]:
        return {"type": "mi355_feedback", "retrieval_unit": self.retrieval_unit, "search_mode": "single", "fb_k": self.fb_k,
                "alpha": self.alpha, "beta": self.beta}

    def _search(self, query_ids: list, top_k: int) -> list[list[dict]]:
        return self._service.vector_search_feedback(query_ids, top_k, fb_k=self.fb_k, alpha=self.alpha, beta=self.beta,
                                                    unit=self.retrieval_unit)

    async def _retrieve_by_id(self, query_id, top_k: int) -> list[dict[str, Any]]:
        results = self._search([query_id], top_k)
        return results[0] if results else []

    async def _retrieve_by_text(self, query_text: str, top_k: int) -> list[dict[str, Any]]:
        if self._embedding_model is None:
            raise EmbeddingError
        query_embedding = await self._service.on_root(lambda: self._embedding_model.aembed_query(query_text))
        return self._service.vector_search_feedback_by_embedding(query_embedding, top_k, fb_k=self.fb_k, alpha=self.alpha,
                                                                 beta=self.beta, unit=self.retrieval_unit)

    def _retrieve_block(self, query_ids: list, top_k: int) -> list[list[dict] | None]:
        """One GPU block for the whole page; a query that cannot be scored (missing row / embedding) fails alone."""
        ok, bad = [], set()
        for qid, q in zip(query_ids, self._service.get_queries(list(query_ids)), strict=True):
            if q is not None and q.embedding is not None:
                ok.append(qid)
            else:
                bad.add(qid)
        res = self._search(ok, top_k) if ok else []
        by_id = dict(zip(ok, res))
        for qid in bad:
            logger.error(f"Retrieval failed for query {qid}")
        return [None if qid in bad else by_id[qid] for qid in query_ids]


__all__ = ["Mi355FeedbackPipelineConfig", "Mi355FeedbackRetrievalPipeline"]
