"""CPU: the mutable sparse store's ABI names, the Python methods' argument checks, and the service taking a refresh of the BM25
leg as the difference alone -- over a host stand-in (tests/sparse_ref.py plus set_sparse / remove_sparse), no GPU."""

import copy
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import sparse_ref
from helpers import OracleIndex, build_golden_stores

ROOT = Path(__file__).resolve().parent.parent
UPDATE_SYMBOLS = ["mi355dr_set_sparse", "mi355dr_remove_sparse", "mi355dr_live_sparse"]


def test_update_symbols_are_declared_listed_and_bound(native_built):
    from autorag_research_amd import _native
    from autorag_research_amd.index import Mi355Index

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mi355dr.h").read_text(), flags=re.S)
    lib = _native.load()
    for name in UPDATE_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _native.ABI_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.mi355dr_set_sparse.argtypes) == 5 and len(lib.mi355dr_remove_sparse.argtypes) == 3
    assert list(inspect.signature(Mi355Index.set_sparse).parameters) == ["self", "doc_ids", "token_lists", "offsets"]
    assert inspect.signature(Mi355Index.set_sparse).parameters["offsets"].default is None
    assert list(inspect.signature(Mi355Index.remove_sparse).parameters) == ["self", "doc_ids"]
    assert callable(Mi355Index.live_sparse)
    full = (ROOT / "include" / "mi355dr.h").read_text()
    assert "update / remove / compact of sparse documents" not in full      # no longer out of scope


class _Recorder:
    """the library as far as the argument checks go: records what would have reached it"""

    def __init__(self):
        self.calls = []

    def mi355dr_set_sparse(self, h, ids, terms, offsets, n):
        self.calls.append(("set", [ids[i] for i in range(n)], [offsets[i] for i in range(n + 1)], [terms[i] for i in range(offsets[n])]))
        return 0

    def mi355dr_remove_sparse(self, h, ids, n):
        self.calls.append(("remove", [ids[i] for i in range(n)]))
        return 0

    def mi355dr_live_sparse(self, h):
        return 7


def test_python_methods_and_their_argument_errors():
    from autorag_research_amd.index import Mi355Index

    ix = Mi355Index.__new__(Mi355Index)                    # no handle, no device: the checks run before the library is called
    ix._lib, ix._h = _Recorder(), None
    ix.set_sparse([4, 2], [[5, 5, 1], []])
    ix.set_sparse(np.array([9]), [7, 8, 9], offsets=[0, 3])                  # the flat form of add_sparse
    ix.remove_sparse((3, 1))
    ix.set_sparse([], [])
    ix.remove_sparse([])
    assert ix._lib.calls == [("set", [4, 2], [0, 3, 3], [5, 5, 1]), ("set", [9], [0, 3], [7, 8, 9]), ("remove", [3, 1]),
                             ("set", [], [0], []), ("remove", [])]
    assert ix.live_sparse() == 7
    for bad in (lambda: ix.set_sparse([1, 2], [[1]]),                        # one id per token list
                lambda: ix.set_sparse([1], [[1], [2]]),
                lambda: ix.set_sparse([1.5], [[1]]),                         # ids are integers
                lambda: ix.remove_sparse([0.5]),
                lambda: ix.set_sparse([1], [1, 2], offsets=[0, 1]),          # offsets end at the number of tokens
                lambda: ix.set_sparse([1, 2], [1, 2], offsets=[0, 2, 1]),    # ... and never decrease
                lambda: ix.set_sparse([1], [[2 ** 31]])):                    # token ids fit int32
        with pytest.raises(ValueError):
            bad()
    assert len(ix._lib.calls) == 5


# ---- the service over a stand-in that can be mutated --------------------------------------------------------------------------

@sparse_ref.sparse_methods
class MutableSparseIndex(OracleIndex):
    """tests/helpers.py's stand-in with sparse_ref's sparse methods, plus set_sparse / remove_sparse over its SparseCorpus"""

    log = []

    def set_sparse(self, doc_ids, token_lists, offsets=None):
        assert offsets is None
        MutableSparseIndex.log.append(("set", id(self), [int(i) for i in doc_ids]))
        for i, d in zip(doc_ids, token_lists, strict=True):
            self._sparse.docs[int(i)] = [int(t) for t in d]
        self._sparse.add([])                               # (derives lengths, N and the postings again)

    def remove_sparse(self, doc_ids):
        self.set_sparse(doc_ids, [[] for _ in doc_ids])


# (sparse_methods installs its add_sparse over the class: the recording one goes on afterwards)
def _recording_add(self, token_lists, offsets=None):
    assert offsets is None
    MutableSparseIndex.log.append(("add", id(self), len(token_lists)))
    if getattr(self, "_sparse", None) is None:
        self._sparse = sparse_ref.SparseCorpus()
    self._sparse.add(token_lists)


MutableSparseIndex.add_sparse = _recording_add


class _CountingTokenizer:
    def __init__(self):
        self.texts = []

    def __call__(self, text):
        from autorag_research_amd.bm25 import simple_tokenizer

        self.texts.append(text)
        return simple_tokenizer(text)


@pytest.fixture()
def svc(monkeypatch, oracle):
    import autorag_research_amd.service as service

    monkeypatch.setattr(service, "Mi355Index", MutableSparseIndex)
    MutableSparseIndex.log = []
    store, g = build_golden_stores()
    s = service.Mi355RetrievalService(lambda: store)
    yield s, store, g
    s.close()


def _expected(table, text, top_k):
    from autorag_research_amd.bm25 import simple_tokenizer

    corpus = sparse_ref.SparseCorpus([[] if c is None else simple_tokenizer(c) for c in table.contents])
    dist, rows = sparse_ref.search_bm25(corpus, [simple_tokenizer(text)], top_k)
    return [{"doc_id": table.ids[r], "score": -d, "content": table.contents[r]} for d, r in zip(dist[0].tolist(), rows[0].tolist()) if r >= 0]


def _grown(table, changes, appended):
    """a newer export: `changes` {position: contents}, `appended` rows at the end (every column follows)"""
    new = copy.copy(table)
    new.contents = list(table.contents)
    for i, c in changes.items():
        new.contents[i] = c
    n = len(appended)
    if n:
        new.contents += list(appended)
        new.ids = list(table.ids) + [f"new-{j}" for j in range(n)]
        for name in ("embedding",):
            col = getattr(table, name, None)
            if col is not None:
                setattr(new, name, np.concatenate([col, np.repeat(col[-1:], n, axis=0)]))
    return new


def test_refresh_with_a_cell_that_became_none(svc):
    s, store, g = svc
    tok = _CountingTokenizer()
    u = s._unit("chunk")
    first = u.ensure_sparse(tok)
    n = len(u.table.contents)
    assert len(tok.texts) == sum(c is not None for c in u.table.contents) and MutableSparseIndex.log == [("add", id(first), n)]
    table = _grown(u.table, {1: "entirely new words here", 4: None}, ["one appended row of words"])
    s.refresh_unit("chunk", table)
    tok.texts.clear()
    MutableSparseIndex.log.clear()
    again = u.ensure_sparse(tok)
    assert again is first and u.sparse is first                                      # the same store object is kept
    assert MutableSparseIndex.log == [("set", id(first), [1, 4]), ("add", id(first), 1)]   # ONE set of those two, ONE add of one
    assert tok.texts == ["entirely new words here", "one appended row of words"]    # None -> no tokens, without a tokeniser call
    assert first.size_sparse() == n + 1
    for text in ("entirely new words", "appended row", g["contents"][3], g["contents"][4] or "nothing"):
        assert s.bm25_search_by_text(text, 5, tokenizer=tok) == _expected(table, text, 5)
    assert s.bm25_search_by_text("entirely new words", 3, tokenizer=tok)[0]["doc_id"] == table.ids[1]
    assert s.bm25_search_by_text("appended row", 3, tokenizer=tok)[0]["doc_id"] == "new-0"
    # the same contents again: nothing is tokenised, nothing is called
    tok.texts.clear()
    MutableSparseIndex.log.clear()
    same_again = _grown(table, {}, [])
    s.refresh_unit("chunk", same_again)
    assert u.ensure_sparse(tok) is first and MutableSparseIndex.log == [] and tok.texts == []


def test_refresh_is_applied_as_the_difference(svc):
    s, store, g = svc
    tok = _CountingTokenizer()
    u = s._unit("chunk")
    first = u.ensure_sparse(tok)
    table = _grown(u.table, {0: "alpha beta", 2: "gamma delta"}, ["epsilon zeta"])
    s.refresh_unit("chunk", table)
    tok.texts.clear()
    MutableSparseIndex.log.clear()
    assert u.ensure_sparse(tok) is first
    assert MutableSparseIndex.log == [("set", id(first), [0, 2]), ("add", id(first), 1)]
    assert tok.texts == ["alpha beta", "gamma delta", "epsilon zeta"]                # only three tokeniser calls
    for text in ("alpha beta", "gamma", "zeta epsilon", g["contents"][3]):
        assert s.bm25_search_by_text(text, 4, tokenizer=tok) == _expected(table, text, 4)


def test_a_shorter_table_or_another_tokeniser_still_rebuilds(svc):
    s, store, g = svc
    tok = _CountingTokenizer()
    u = s._unit("chunk")
    first = u.ensure_sparse(tok)
    other = _CountingTokenizer()
    second = u.ensure_sparse(other)                                                  # another tokenizer: a new store
    assert second is not first and len(other.texts) == sum(c is not None for c in u.table.contents)
    shorter = copy.copy(u.table)
    shorter.contents = list(u.table.contents)[:-1]
    shorter.ids = list(u.table.ids)[:-1]
    if getattr(shorter, "embedding", None) is not None:
        shorter.embedding = shorter.embedding[:-1]
    s.refresh_unit("chunk", shorter)
    MutableSparseIndex.log.clear()
    third = u.ensure_sparse(other)
    assert third is not second and MutableSparseIndex.log == [("add", id(third), len(shorter.contents))]
    assert s.bm25_search_by_text(g["contents"][2], 3, tokenizer=other) == _expected(shorter, g["contents"][2], 3)
