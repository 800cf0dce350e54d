"""CPU: the row-sharded sparse forms' declaration and binding, `ShardedSearcher`'s sparse methods over stand-in indexes
(delegation at world size 1, the refusal of another shard's ids), and the service's opt-in `shard_sparse` path over host
stand-ins and a fake two-rank world -- with the default argument the service calls exactly what it called before."""

import copy
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import sparse_ref
import sparse_shard_ref
import sparse_subset_ref
from helpers import OracleIndex, build_golden_stores

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = {"mi355dr_search_sparse_sharded_device": "mi355dr_search_sparse_device",
           "mi355dr_search_bm25_sharded_device": "mi355dr_search_bm25_device",
           "mi355dr_search_sparse_subset_sharded_device": "mi355dr_search_sparse_subset_device",
           "mi355dr_search_bm25_subset_sharded_device": "mi355dr_search_bm25_subset_device",
           "mi355dr_score_sparse_subset_sharded": "mi355dr_score_sparse_subset",
           "mi355dr_score_bm25_subset_sharded": "mi355dr_score_bm25_subset"}
METHODS = ("search_bm25", "search_sparse", "search_bm25_subset", "search_sparse_subset", "score_bm25_subset", "score_sparse_subset")


def test_header_declares_library_exports_and_native_binds(native_built):
    full = (ROOT / "include" / "mi355dr.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    from autorag_research_amd import _native

    lib = _native.load()
    for name, local in SYMBOLS.items():
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert name in _native.ABI_SYMBOLS
        assert list(getattr(lib, name).argtypes) == list(getattr(lib, local).argtypes), name   # the local form's arguments
    # the declarations stand behind the derived sharded searches, and the sparse section no longer calls the search missing
    assert text.index("mi355dr_mmr_select_sharded") < text.index("mi355dr_search_sparse_sharded_device") < text.index("mi355dr_set_option")
    assert "a row-sharded sparse search (it needs" not in full and "row-sharded sparse search" in full
    assert "SAME libm" in full and "row-sharded hybrids" in full
    from autorag_research_amd.index import Mi355Index

    for m in METHODS:
        local = inspect.signature(getattr(Mi355Index, m)).parameters
        sharded = inspect.signature(getattr(Mi355Index, m + "_sharded")).parameters
        assert list(sharded) == [p for p in local if p != "device_out"], m
    for m in METHODS[:4]:
        assert callable(getattr(Mi355Index, m + "_sharded_device")), m


# ---- ShardedSearcher over a recording stand-in ------------------------------------------------------------------------------

class Recorder:
    """an index stand-in that records the local calls and has none of the sharded entry points"""

    def __init__(self, dim, metric="cosine", device=0):
        self.dim, self.calls, self.options, self.n_sparse = dim, [], {}, 0

    def set_option(self, key, value):
        self.options[key] = value

    def size_sparse(self):
        return self.n_sparse

    def add_sparse(self, docs):
        self.calls.append(("add_sparse", (docs,)))
        self.n_sparse += len(docs)

    def close(self):
        pass


def _record(name):
    def method(self, *args, **kw):
        assert not kw
        self.calls.append((name, args))
        return name

    return method


for _m in METHODS + ("set_sparse", "remove_sparse"):
    setattr(Recorder, _m, _record(_m))

ARGS = {
    "search_bm25": ([[1, 2], [3]], 5, 0.9, 0.4),
    "search_sparse": ([1, 2, 3], [1.0, 0.5, 2.0], [0, 2, 3], 5, 0.9, 0.4),
    "search_bm25_subset": ([[1, 2], [3]], 5, np.array([4, 9]), 0.9, 0.4),
    "search_sparse_subset": ([1, 2, 3], [1.0, 0.5, 2.0], [0, 2, 3], 5, np.array([4, 9]), 0.9, 0.4),
    "score_bm25_subset": ([[1, 2], [3]], np.array([[4, 9], [1, 1]]), 0.9, 0.4),
    "score_sparse_subset": ([1, 2, 3], [1.0, 0.5, 2.0], [0, 2, 3], np.array([[4, 9], [1, 1]]), 0.9, 0.4),
}


@pytest.mark.parametrize("method", METHODS)
def test_world_one_delegates_to_the_local_method_with_the_arguments_unchanged(method):
    from autorag_research_amd.sharded import ShardedSearcher

    s = ShardedSearcher(4, index_factory=Recorder)
    assert s.world == 1
    assert getattr(s, method)(*ARGS[method]) == method
    (name, args), = s.index.calls
    assert name == method and len(args) == len(ARGS[method]) and all(a is b for a, b in zip(args, ARGS[method]))
    del s.index.calls[:]
    getattr(s, method)(*ARGS[method][:-2])                   # the defaults of the local methods
    assert s.index.calls[0][1][-2:] == (1.2, 0.75)


@pytest.mark.parametrize("method", METHODS)
def test_force_pipeline_without_the_sharded_entry_points_is_not_implemented(method):
    from autorag_research_amd.sharded import ShardedSearcher

    s = ShardedSearcher(4, index_factory=Recorder)
    s.force_pipeline = True
    with pytest.raises(NotImplementedError, match=method):
        getattr(s, method)(*ARGS[method])
    assert s.index.calls == []


def test_local_mutations_take_global_ids_and_refuse_another_shards():
    from autorag_research_amd.sharded import ShardedSearcher

    s = ShardedSearcher(4, index_factory=Recorder)
    s.add_local_sparse([[1], [2], [3]], 100)
    assert s.row_offset == 100 and s.index.options == {"row_offset": 100}
    s.add_local_sparse([[4]], 555)                              # (set once: a later add appends behind the first)
    assert s.row_offset == 100 and s.index.size_sparse() == 4
    del s.index.calls[:]
    s.set_local_sparse([103, 100], [[7], [8]])
    s.remove_local_sparse(np.array([101]))
    (n1, a1), (n2, a2) = s.index.calls
    assert n1 == "set_sparse" and a1[0].tolist() == [3, 0] and a1[1] == [[7], [8]]
    assert n2 == "remove_sparse" and a2[0].tolist() == [1]
    del s.index.calls[:]
    for bad in ([99], [104], [100, 2000], [-1]):
        with pytest.raises(ValueError, match=r"outside this shard \[100, 104\)"):
            s.set_local_sparse(bad, [[1]] * len(bad))
        with pytest.raises(ValueError, match="remove_local_sparse"):
            s.remove_local_sparse(bad)
    assert s.index.calls == []


def test_one_searcher_holds_one_id_space():
    from autorag_research_amd.sharded import ShardedSearcher

    class WithRows(Recorder):
        def __len__(self):
            return 5

    s = ShardedSearcher(4, index_factory=WithRows)
    s.row_offset = 40                                           # (as add_local leaves it)
    with pytest.raises(ValueError, match="a searcher of their own"):
        s.add_local_sparse([[1]], 100)
    assert s.row_offset == 40 and s.index.options == {} and s.index.calls == []
    s.add_local_sparse([[1]], 40)                               # the same id space: fine
    assert s.index.size_sparse() == 1


# ---- the service: default unchanged, `shard_sparse=True` under a fake world ----------------------------------------------

@sparse_subset_ref.sparse_subset_methods
class SubsetOracleIndex(OracleIndex):
    """the stand-in of tests/helpers.py with the sparse and the *_subset methods answered by the references"""


class FakeWorld:
    """what the service asks of a _World on the paths under test; no process group"""

    group = None

    def __init__(self, rank, size):
        self.rank, self.size = rank, size

    def from_root(self, make):
        return make()

    def same_everywhere(self, what, value):
        pass


class FakeShardedSearcher:
    """ShardedSearcher's sparse surface for a fake world: every instance holds its rank's documents, and a search is answered
    by tests/sparse_shard_ref.py over the slices of ALL instances alive -- what the library's sharded forms return."""

    alive: list = []
    log: list = []

    def __init__(self, dim, metric="cosine", device=0, index_factory=None, group=None):
        self.corpus, self.row_offset, self.factory = sparse_ref.SparseCorpus(), None, index_factory
        FakeShardedSearcher.alive.append(self)

    def add_local_sparse(self, docs, global_doc0):
        assert self.row_offset is None
        self.row_offset = int(global_doc0)
        self.corpus.add(docs)
        FakeShardedSearcher.log.append(("add_local_sparse", self.row_offset, len(docs)))

    def set_local_sparse(self, doc_ids, docs):
        FakeShardedSearcher.log.append(("set_local_sparse", [int(i) for i in doc_ids]))
        for i, d in zip(doc_ids, docs, strict=True):
            assert 0 <= int(i) - self.row_offset < len(self.corpus)
            self.corpus.docs[int(i) - self.row_offset] = [int(t) for t in d]
        self.corpus.add([])

    def _shards(self):
        shards = sorted(FakeShardedSearcher.alive, key=lambda s: s.row_offset)
        assert [s.row_offset for s in shards] == sparse_shard_ref.shard_offsets([s.corpus for s in shards])   # contiguous slices
        return [s.corpus for s in shards]

    def search_bm25(self, token_lists, k, k1=1.2, b=0.75):
        FakeShardedSearcher.log.append(("search_bm25", len(token_lists), k))
        return sparse_shard_ref.search_bm25(self._shards(), token_lists, k, k1, b)

    def search_bm25_subset(self, token_lists, k, doc_ids, k1=1.2, b=0.75):
        FakeShardedSearcher.log.append(("search_bm25_subset", len(token_lists), k, len(doc_ids)))
        return sparse_shard_ref.search_bm25(self._shards(), token_lists, k, k1, b, doc_ids=doc_ids)

    def score_bm25_subset(self, token_lists, doc_ids, k1=1.2, b=0.75):
        FakeShardedSearcher.log.append(("score_bm25_subset", np.asarray(doc_ids).shape))
        return sparse_shard_ref.score_bm25(self._shards(), token_lists, doc_ids, k1, b)

    def close(self):
        FakeShardedSearcher.alive.remove(self)


@pytest.fixture()
def services(monkeypatch, oracle):
    """(a plain service, two services with shard_sparse=True as ranks 0 and 1 of a fake world, the golden data)"""
    import autorag_research_amd.service as service
    import autorag_research_amd.sharded as sharded

    monkeypatch.setattr(service, "Mi355Index", SubsetOracleIndex)
    monkeypatch.setattr(sharded, "ShardedSearcher", FakeShardedSearcher)
    FakeShardedSearcher.alive, FakeShardedSearcher.log = [], []
    store, g = build_golden_stores()
    plain = service.Mi355RetrievalService(lambda: store)
    ranks = []
    for r in range(2):
        s = service.Mi355RetrievalService(lambda: store, shard_sparse=True)
        s._unit("chunk")
        s._world = FakeWorld(r, 2)
        ranks.append(s)
    yield plain, ranks, g
    for s in [plain] + ranks:
        s._world = None
        s.close()


def test_service_default_calls_what_it_called_before(services):
    import autorag_research_amd.service as service

    plain, ranks, g = services
    p = inspect.signature(service.Mi355RetrievalService.__init__).parameters
    assert p["shard_sparse"].default is False and list(p)[-1] == "shard_sparse"
    text = g["contents"][3]
    full = plain.bm25_search_by_text(text, 5)
    u = plain._unit("chunk")
    assert u.sparse is not None and u.sparse_sharded is None and FakeShardedSearcher.log == []
    # shard_sparse without a world changes nothing either; neither does a world without shard_sparse
    plain._shard_sparse = True
    assert plain.bm25_search_by_text(text, 5) == full and u.sparse_sharded is None
    plain._shard_sparse, plain._world = False, FakeWorld(0, 2)
    try:
        assert plain.bm25_search_by_text(text, 5) == full and u.sparse_sharded is None and FakeShardedSearcher.log == []
        assert plain.bm25_lists_device([text], 5, "simple", 1.2, 0.75) is None
    finally:
        plain._world = None


def test_service_shard_sparse_builds_the_slice_and_goes_through_the_searcher(services):
    from autorag_research_amd.sharded import shard_bounds

    plain, ranks, g = services
    ids = list(g["ids"])
    n = len(ids)
    text = "3 13 57 zzzz 13"
    for s in ranks:                                              # every rank builds its slice before the first search
        s._unit("chunk").sparse_searcher("simple", s._world)
    assert FakeShardedSearcher.log == [("add_local_sparse", *shard_bounds(n, 2, 0)[:1], shard_bounds(n, 2, 0)[1]),
                                       ("add_local_sparse", shard_bounds(n, 2, 1)[0], n - shard_bounds(n, 2, 1)[0])]
    del FakeShardedSearcher.log[:]
    full = plain.bm25_search_by_text(text, n)
    within = [r["doc_id"] for r in full[::2]] + ["no such key"]
    for s in ranks:
        u = s._unit("chunk")
        assert u.sparse is None and u.sparse_sharded is not None
        assert s.bm25_search_by_text(text, 5) == full[:5]                                   # global statistics: the plain answer
        assert s.bm25_search_by_text(text, 4, within=within) == plain.bm25_search_by_text(text, 4, within=within)
        assert s.bm25_search([f"q{i}" for i in range(3)], 4) == plain.bm25_search([f"q{i}" for i in range(3)], 4)
        assert s.bm25_score_candidates(text, ids + ["no such key"]) == plain.bm25_score_candidates(text, ids + ["no such key"])
        assert s.bm25_lists_device([text], 5, "simple", 1.2, 0.75) is None                  # device fusion stays out of scope
        assert u.sparse is None
    kinds = [e[0] for e in FakeShardedSearcher.log]
    assert kinds == ["search_bm25", "search_bm25_subset", "search_bm25", "score_bm25_subset"] * 2


def test_service_shard_sparse_refresh(services):
    plain, ranks, g = services
    n = len(g["ids"])
    plain._unit("chunk")                                         # (a unit nothing was built for would defer the refresh)
    for s in ranks:
        s._unit("chunk").sparse_searcher("simple", s._world)
    first = [s._unit("chunk").sparse_sharded for s in ranks]
    table = copy.copy(ranks[0]._unit("chunk").table)
    table.contents = list(table.contents)
    table.contents[1], table.contents[n - 2] = "entirely new words here", None
    del FakeShardedSearcher.log[:]
    for s in [plain] + ranks:
        s.refresh_unit("chunk", table)
    for s in ranks:
        assert s._unit("chunk").sparse_searcher("simple", s._world) in first                # equal length: the store is kept ...
    assert FakeShardedSearcher.log == [("set_local_sparse", [1]), ("set_local_sparse", [n - 2])]   # ... each cell set on its owner
    want = plain.bm25_search_by_text("entirely new words", 3)
    assert want[0]["doc_id"] == table.ids[1]
    assert [s.bm25_search_by_text("entirely new words", 3) for s in ranks] == [want, want]
    # the same contents again: nothing is called
    del FakeShardedSearcher.log[:]
    again = copy.copy(table)
    again.contents = list(table.contents)
    for s in ranks:
        s.refresh_unit("chunk", again)
        s._unit("chunk").sparse_searcher("simple", s._world)
    assert FakeShardedSearcher.log == []
    # another length: every rank rebuilds its slice
    longer = copy.copy(table)
    longer.contents = list(table.contents) + ["one appended row of words"]
    longer.ids = list(table.ids) + ["new-0"]
    if getattr(table, "embedding", None) is not None:
        longer.embedding = np.concatenate([table.embedding, table.embedding[-1:]])
    for s in [plain] + ranks:
        s.refresh_unit("chunk", longer)
    for s in ranks:
        s._unit("chunk").sparse_searcher("simple", s._world)
    assert [e[0] for e in FakeShardedSearcher.log] == ["add_local_sparse"] * 2 and len(FakeShardedSearcher.alive) == 2
    want = plain.bm25_search_by_text("appended row", 3)
    assert want[0]["doc_id"] == "new-0"
    assert [s.bm25_search_by_text("appended row", 3) for s in ranks] == [want, want]
