"""BM25 retrieval over this package's own stores: the lexical leg of the hybrid pipelines, scored on the MI355X.

Mirrors the reference's BM25PipelineConfig / BM25RetrievalPipeline (pipelines/retrieval/bm25.py:18-171), whose search is
one SQL statement against VectorChord-BM25 (orm/repository/chunk.py:185-247).  Here the chunk table's `contents` are
tokenised on the host, stored in the library's sparse store (include/mi355dr.h "sparse store") and a page of queries is
scored as one block by `Mi355Index.search_bm25`.  The arithmetic is the one that header fixes; agreement with the
reference is on the interface only -- signatures, positive scores with higher = better, result dicts -- never on the
score bits of VectorChord-BM25, and the vocabularies of pg_tokenizer are not reproduced.

Tokenizers are callables `str -> list[int]` with ids in [0, 2^20):

* ``"simple"``: lowercase, ``[0-9a-z]+`` words, id = crc32(word) mod 2^20 (the hashing idiom of rerank.RandomTokenEncoder);
* a directory that holds a Hugging Face tokenizer: loaded with ``local_files_only=True``, no special tokens;
* a hub name such as the reference's default ``"bert"`` is refused with an error that asks for a local directory.
  Nothing is ever fetched.
"""

from __future__ import annotations

import logging
import os
import re
import zlib
from collections.abc import Callable
from dataclasses import dataclass
from typing import Any

from .compat import BaseRetrievalPipelineConfig
from .pipelines import Mi355BaseRetrievalPipeline

logger = logging.getLogger("AutoRAG-Research")

DEFAULT_BM25_INDEX_NAME = "idx_chunk_bm25"  # the reference's default (bm25.py:15); recorded, unused here
TERM_LIMIT = 1 << 20                        # the sparse store's term ids lie in [0, 2^20)
_WORD = re.compile(r"[0-9a-z]+")

Tokenizer = Callable[[str], list[int]]


def simple_tokenizer(text: str) -> list[int]:
    """Lowercase, ``[0-9a-z]+`` words, id = crc32(word) mod 2^20."""
    return [zlib.crc32(w.encode()) % TERM_LIMIT for w in _WORD.findall(text.lower())]


class _HFTokenizer:
    """A Hugging Face tokenizer from a LOCAL directory: its ids without special tokens (ids past 2^20 wrap)."""

    def __init__(self, path: str):
        from transformers import AutoTokenizer  # noqa: PLC0415

        self._tok = AutoTokenizer.from_pretrained(path, local_files_only=True)

    def __call__(self, text: str) -> list[int]:
        return [int(i) % TERM_LIMIT for i in self._tok.encode(text, add_special_tokens=False)]


_LOADED: dict[str, Tokenizer] = {}


def get_tokenizer(tokenizer: str | Tokenizer) -> Tokenizer:
    """The callable behind a tokenizer name (see the module docstring); a callable is returned as it is."""
    if callable(tokenizer):
        return tokenizer
    if tokenizer == "simple":
        return simple_tokenizer
    if isinstance(tokenizer, str) and os.path.isdir(tokenizer):
        if tokenizer not in _LOADED:
            _LOADED[tokenizer] = _HFTokenizer(tokenizer)
        return _LOADED[tokenizer]
    raise ValueError(
        f"BM25 tokenizer {tokenizer!r} is neither 'simple' nor a local directory: pg_tokenizer's pre-built models "
        "('bert', 'wiki_tocken', ...) and hub names are not downloaded here -- pass the path of a directory that holds "
        "the Hugging Face tokenizer's files, or 'simple'")


def tokenizer_key(tokenizer: str | Tokenizer) -> Any:
    """What identifies a tokenizer for a cached sparse store: its name, or the callable itself."""
    return tokenizer if isinstance(tokenizer, str) else id(tokenizer)


@dataclass(kw_only=True)
class Mi355BM25PipelineConfig(BaseRetrievalPipelineConfig):
    """Fields as BM25PipelineConfig (bm25.py:18-65) + the BM25 parameters and `device`.  `tokenizer` defaults to "simple":
    the reference's default "bert" names a pg_tokenizer model that cannot be had without a download."""

    tokenizer: str = "simple"
    index_name: str = DEFAULT_BM25_INDEX_NAME
    k1: float = 1.2
    b: float = 0.75
    device: int = 0

    def get_pipeline_class(self) -> type["Mi355BM25RetrievalPipeline"]:
        return Mi355BM25RetrievalPipeline

    def get_pipeline_kwargs(self) -> dict[str, Any]:
        return {"tokenizer": self.tokenizer, "index_name": self.index_name, "k1": self.k1, "b": self.b, "device": self.device}


class Mi355BM25RetrievalPipeline(Mi355BaseRetrievalPipeline):
    """BM25 over the chunk table's contents, scored by the library's sparse store (reference BM25RetrievalPipeline,
    bm25.py:68-171).  A valid child of Mi355HybridRRF / Mi355HybridCC / Mi355GQRHybrid, which take instances."""

    retrieval_unit = "chunk"

    def __init__(self, session_factory: Any, name: str, tokenizer: str | Tokenizer = "simple",
                 index_name: str = DEFAULT_BM25_INDEX_NAME, k1: float = 1.2, b: float = 0.75, schema: Any | None = None,
                 device: int = 0):
        # set BEFORE super().__init__: _get_pipeline_config() is called there (bm25.py:126-131)
        self.tokenizer = tokenizer
        self.index_name = index_name
        self.k1 = k1
        self.b = b
        get_tokenizer(tokenizer)  # (a name that cannot be served fails here, not at the first query)
        super().__init__(session_factory, name, schema, device=device)

    def _get_pipeline_config(self) -> dict[str, Any]:
        name = self.tokenizer if isinstance(self.tokenizer, str) else getattr(self.tokenizer, "__name__", "callable")
        return {"type": "bm25", "retrieval_unit": self.retrieval_unit, "tokenizer": name, "index_name": self.index_name,
                "k1": self.k1, "b": self.b}

    def _kw(self) -> dict[str, Any]:
        return {"tokenizer": self.tokenizer, "index_name": self.index_name, "k1": self.k1, "b": self.b}

    async def _retrieve_by_id(self, query_id: int | str, top_k: int) -> list[dict[str, Any]]:
        results = self._service.bm25_search([query_id], top_k, **self._kw())
        return results[0] if results else []

    async def _retrieve_by_text(self, query_text: str, top_k: int) -> list[dict[str, Any]]:
        return self._service.bm25_search_by_text(query_text, top_k, **self._kw())

    def _retrieve_block(self, query_ids: list, top_k: int) -> list[list[dict] | None]:
        """One block for the whole page; a query without a row (or without text) fails alone."""
        ok, bad = [], set()
        for qid, q in zip(query_ids, self._service.get_queries(list(query_ids)), strict=True):
            if q is not None and q.contents is not None:
                ok.append(qid)
            else:
                bad.add(qid)
        res = self._service.bm25_search(ok, top_k, **self._kw()) if ok else []
        by_id = dict(zip(ok, res))
        for qid in bad:
            logger.error(f"Retrieval failed for query {qid}")
        return [None if qid in bad else by_id[qid] for qid in query_ids]


__all__ = ["DEFAULT_BM25_INDEX_NAME", "Mi355BM25PipelineConfig", "Mi355BM25RetrievalPipeline", "TERM_LIMIT", "get_tokenizer",
           "simple_tokenizer", "tokenizer_key"]
