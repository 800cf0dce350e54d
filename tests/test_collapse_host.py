"""CPU: the host layers of the source cap -- the binding's prototypes, `ShardedSearcher.search_collapsed` over a stand-in, and
the service's `per_source` arguments: their checks, and the key table it builds in the id space of each leg (a dense index's
rows are not table positions once a chunk has no embedding), over an oracle-backed index whose "device memory" is a dict."""

import re
from pathlib import Path

import numpy as np
import pytest

import collapse_ref as cr
from test_subset_host import OracleSubsetIndex

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("mi355dr_collapse_lists_device", "mi355dr_collapse_lists", "mi355dr_search_collapsed", "mi355dr_search_collapsed_device",
         "mi355dr_search_collapsed_sharded_device")


def test_header_declares_library_exports_and_native_binds(native_built):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mi355dr.h").read_text(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    assert re.search(r"#define\s+MI355DR_COLLAPSE_TRUNCATED\s+1\b", text)
    from autorag_research_amd import _native, index

    assert set(NAMES) <= set(_native.ABI_SYMBOLS)
    lib = _native.load()
    assert [len(getattr(lib, name).argtypes) for name in NAMES] == [16, 15, 14, 15, 15]
    # the arguments of each prototype, counted in the header itself
    for name in NAMES:
        decl = re.search(rf"\bint\s+{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(decl.split(",")) == len(getattr(lib, name).argtypes), name
    assert index.COLLAPSE_TRUNCATED == 1
    for m in ("collapse_lists", "collapse_lists_device", "search_collapsed", "search_collapsed_device",
              "search_collapsed_sharded_device", "search_collapsed_sharded", "search_maxsim_collapsed", "search_bm25_collapsed",
              "upload_keys"):
        assert callable(getattr(index.Mi355Index, m)), m
    f = index.Mi355Index.collapse_fetch_k
    assert f(10, None, 1024) == index.COLLAPSE_FETCH_MULT * 10 and f(10, 37, 1024) == 37
    assert f(1000, None, 1024) == min(1024, index.COLLAPSE_FETCH_MULT * 1000) and f(10, None, 10) == 10


def test_every_stat_of_the_section_is_in_the_header():
    text = (ROOT / "include" / "mi355dr.h").read_text()
    for stat in ("collapse_calls", "collapse_searches", "collapse_queries", "collapse_researched", "collapse_truncated"):
        assert text.count(f'"{stat}"') >= 2, stat


# ---- ShardedSearcher ----------------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self, dim, metric="cosine", device=0):
        self.dim, self.calls = dim, []

    def __len__(self):
        return 0

    def set_option(self, key, value):
        pass

    def close(self):
        pass

    def search_collapsed(self, *args):
        self.calls.append(args)
        return "local"


def test_sharded_searcher_delegates_at_world_one_and_refuses_an_index_without_the_sharded_form():
    from autorag_research_amd.sharded import ShardedSearcher

    s = ShardedSearcher(4, index_factory=Recorder)
    Q, keys = np.zeros((2, 4), np.float32), np.arange(5)
    assert s.search_collapsed(Q, 3, 2, keys, 9, 64) == "local"
    assert s.search_collapsed(Q, 3, 2, keys) == "local"
    (a, b) = s.index.calls
    assert a[0] is Q and a[3] is keys and a[1:3] == (3, 2) and a[4:] == (9, 64) and b[4:] == (None, 1024)
    s.force_pipeline = True
    with pytest.raises(NotImplementedError, match="search_collapsed"):
        s.search_collapsed(Q, 3, 2, keys)
    assert len(s.index.calls) == 2


# ---- the service ----------------------------------------------------------------------------------------------------------------
class HostIndex(OracleSubsetIndex):
    """The oracle-backed stand-in + the source cap by tests/collapse_ref.py, over "device memory" kept in a dict: what the
    service uploads as a key table is what the cap reads."""

    memory: dict = {}
    uploads: list = []

    @staticmethod
    def collapse_fetch_k(k, fetch_k, max_fetch):
        from autorag_research_amd.index import Mi355Index

        return Mi355Index.collapse_fetch_k(k, fetch_k, max_fetch)

    def dev_alloc(self, nbytes):
        ptr = 4096 * (len(HostIndex.memory) + 1)
        HostIndex.memory[ptr] = None
        return ptr

    def dev_free(self, ptr):
        del HostIndex.memory[ptr]

    def dev_upload(self, ptr, arr):
        HostIndex.memory[ptr] = np.array(arr, copy=True)
        HostIndex.uploads.append(ptr)

    def _table(self, keys):
        from autorag_research_amd.index import DeviceKeys

        assert isinstance(keys, DeviceKeys)            # the service keeps the table on the device
        if keys.length == 0:
            return None
        t = HostIndex.memory[keys.ptr]
        assert t.dtype == np.int64 and t.shape == (keys.length,)
        return t

    def collapse_lists(self, vals, ids, keys, cap, k=None, **kw):
        from autorag_research_amd.index import CollapsedLists

        c = cr.collapse(vals, ids, self._table(keys), cap, np.asarray(ids).shape[1] if k is None else k)
        return CollapsedLists(c.vals, c.ids, c.keys, c.pos, c.count, c.entries)

    def search_collapsed(self, queries, k, cap, keys, fetch_k=None, max_fetch=1024):
        from autorag_research_amd.index import CollapsedSearch

        self.last_fetch_k = fetch_k
        d, r = self.search(queries, max_fetch)
        return CollapsedSearch(*cr.search_result(d, r, self._table(keys), cap, k, max_fetch))


@pytest.fixture()
def env(monkeypatch, oracle):
    import autorag_research_amd.service as svc
    from autorag_research_amd.store import InMemoryStore

    monkeypatch.setattr(svc, "Mi355Index", HostIndex)
    HostIndex.memory, HostIndex.uploads = {}, []
    rng = np.random.default_rng(12)
    n, d, dm = 60, 16, 8
    C = rng.standard_normal((n, d)).astype(np.float32)
    nulls = [0, 7, 8, 30]                              # chunks without an embedding: index rows are not table positions
    C[nulls] = np.nan
    docs = [rng.standard_normal((int(t), dm)).astype(np.float32) for t in rng.integers(1, 6, size=n)]
    docs[5] = None
    ids = [f"c{i:02d}" for i in range(n)]
    store = InMemoryStore()
    store.set_chunks(ids, [f"text {i}" for i in range(n)], embedding=C, multivec=docs)
    Q = rng.standard_normal((3, d)).astype(np.float32)
    Qm = [rng.standard_normal((t, dm)).astype(np.float32) for t in (2, 4, 1)]
    store.add_queries(["q0", "q1", "q2"], contents=["a", "b", "c"], embedding=list(Q), embeddings=Qm)
    source_of = {pk: f"doc{i // 6}" for i, pk in enumerate(ids) if i % 10 != 9}   # every tenth chunk has no source
    return svc.Mi355RetrievalService(lambda: store), dict(ids=ids, nulls=nulls, Q=Q, source_of=source_of, n=n)


def _capped(results, source_of, cap, k):
    """the reference over a service result list: at most `cap` per source, in list order, the first k"""
    seen, out = {}, []
    for r in results:
        src = source_of.get(r["doc_id"])
        if src is not None:
            seen[src] = seen.get(src, 0) + 1
            if seen[src] > cap:
                continue
        out.append(r)
    return out[:k]


def test_source_key_table_in_each_id_space():
    from autorag_research_amd.service import source_key_table

    ids = ["a", "b", "c", "d", "e"]
    source_of = {"a": "x", "b": "y", "d": "x", "e": None, "zz": "unused"}
    assert source_key_table(ids, source_of).tolist() == [0, 1, -1, 0, -1]             # numbered in first-seen table order
    assert source_key_table(ids, source_of, np.array([1, 3, 4])).tolist() == [1, 0, -1]   # index rows 0 1 2 = positions 1 3 4
    assert source_key_table(ids, {}).tolist() == [-1] * 5 and source_key_table([], source_of).shape == (0,)
    assert source_key_table(ids, source_of).dtype == np.int64


def test_per_source_single_uses_rows_not_positions(env):
    s, e = env
    q = [float(x) for x in e["Q"][1]]
    full = s.vector_search_by_embedding(q, e["n"])
    assert len(full) == e["n"] - len(e["nulls"])
    for cap in (2, 1):
        got = s.vector_search_by_embedding(q, 8, per_source=cap, source_of=e["source_of"])
        assert got == _capped(full, e["source_of"], cap, 8)
    assert got != full[:8]                               # not vacuous: at one per source the cap struck something
    # the table the service uploaded is indexed by INDEX ROW: row j is the j-th chunk WITH an embedding
    u = s._unit("chunk")
    table = HostIndex.memory[u._source_keys["single"].ptr]
    with_emb = [i for i in range(e["n"]) if i not in e["nulls"]]
    assert table.shape == (len(with_emb),)
    codes = {}
    expect = [codes.setdefault(e["source_of"][e["ids"][i]], len(codes)) if e["ids"][i] in e["source_of"] else -1 for i in range(e["n"])]
    assert table.tolist() == [expect[i] for i in with_emb] and -1 in table.tolist()
    # uploaded once per mapping: the same object again costs no upload, a new mapping does
    n_up = len(HostIndex.uploads)
    s.vector_search(["q0", "q1", "q2"], 5, per_source=1, source_of=e["source_of"])
    assert len(HostIndex.uploads) == n_up
    s.vector_search(["q0"], 5, per_source=1, source_of=dict(e["source_of"]))
    assert len(HostIndex.uploads) == n_up + 1
    # the block form equals the single form, query by query; source_fetch_k reaches the search
    blocks = s.vector_search(["q0", "q1", "q2"], 6, per_source=1, source_of=e["source_of"], source_fetch_k=20)
    assert u.single.last_fetch_k == 20
    for b, got in enumerate(blocks):
        one = s.vector_search_by_embedding([float(x) for x in e["Q"][b]], e["n"])
        assert got == _capped(one, e["source_of"], 1, 6)


def test_per_source_within_and_multi(env):
    s, e = env
    q = [float(x) for x in e["Q"][2]]
    within = [pk for i, pk in enumerate(e["ids"]) if i % 3 != 1] + ["nope"]
    depth = 24
    base = s.vector_search_by_embedding(q, depth, within=within)
    got = s.vector_search_by_embedding(q, 5, within=within, per_source=1, source_of=e["source_of"], source_fetch_k=depth)
    assert got == _capped(base, e["source_of"], 1, 5) and got != base[:5]
    base_m = s.vector_search(["q0", "q1", "q2"], 30, "multi")
    got_m = s.vector_search(["q0", "q1", "q2"], 6, "multi", per_source=1, source_of=e["source_of"], source_fetch_k=30)
    assert got_m == [_capped(b, e["source_of"], 1, 6) for b in base_m]
    assert any(g != b[:6] for g, b in zip(got_m, base_m))
    u = s._unit("chunk")
    assert HostIndex.memory[u._source_keys["multi"].ptr].shape == (e["n"],)      # a multi-vector store's ids are positions
    # the default depth is the index's rule
    got_d = s.vector_search(["q1"], 4, "multi", per_source=2, source_of=e["source_of"])
    import autorag_research_amd.service as svc

    depth = svc.LIST_SOURCE_FETCH_MULT * 4            # the list-capped legs do not deepen: their default is their own
    assert s._source_depth(4, None) == depth > 4 and s._source_depth(4, 9) == 9 and s._source_depth(1000, None) == 1024
    assert got_d == [_capped(s.vector_search(["q1"], depth, "multi")[0], e["source_of"], 2, 4)]


def test_per_source_argument_checks(env):
    s, e = env
    q = [float(x) for x in e["Q"][0]]
    so = e["source_of"]
    for kw in (dict(per_source=0, source_of=so), dict(per_source=-1, source_of=so), dict(per_source=1.5, source_of=so),
               dict(per_source=True, source_of=so), dict(per_source=1), dict(per_source=1, source_of=["c00"]),
               dict(per_source=1, source_of=so, source_fetch_k=4), dict(per_source=1, source_of=so, source_fetch_k=1025),
               dict(per_source=1, source_of=so, mmr_fetch_k=20)):
        with pytest.raises(ValueError):
            s.vector_search_by_embedding(q, 5, **kw)
        with pytest.raises(ValueError):
            s.vector_search(["q0"], 5, **kw)
    with pytest.raises(ValueError):
        s.maxsim_search_by_embeddings([e["Q"][:1]], 5, per_source=0, source_of=so)
    with pytest.raises(ValueError):
        s.bm25_search_by_text("text", 5, per_source=1)
    with pytest.raises(ValueError):
        s.bm25_search(["q0"], 5, per_source=2, source_of=so, source_fetch_k=3)
    # per_source=None is today's behaviour, whatever else is passed
    assert s.vector_search_by_embedding(q, 5, source_of=so, source_fetch_k=2) == s.vector_search_by_embedding(q, 5)


# ---- the service under a _World: the sharded searcher's `.index` is the handle, the key table is over GLOBAL rows ----------------
class FakeWorld:
    """what the service asks of a _World on the paths under test; no process group"""

    group = None

    def __init__(self, rank, size):
        self.rank, self.size = rank, size

    def from_root(self, make):
        return make()

    def same_everywhere(self, what, value):
        pass


class FakeSharded:
    """ShardedSearcher's dense surface for a fake world: every instance holds its rank's rows behind an `.index` of its own
    (the handle the service uploads through), and a search is answered over the rows of ALL instances alive, in global row
    order -- what the library's sharded forms return on every rank.  No `collapse_lists` of its own: the service must go to
    `.index` for the list form."""

    alive: list = []
    log: list = []

    def __init__(self, dim, metric="cosine", device=0, index_factory=None, group=None):
        self.dim, self.metric, self.index, self.row_offset, self.rows = dim, metric, index_factory(dim, metric, device), None, None
        FakeSharded.alive.append(self)

    def add_local(self, rows, row0):
        self.rows, self.row_offset = np.ascontiguousarray(rows, dtype=np.float32), int(row0)

    def _whole(self):
        shards = sorted(FakeSharded.alive, key=lambda s: s.row_offset)
        assert [s.row_offset for s in shards] == np.cumsum([0] + [len(s.rows) for s in shards])[:-1].tolist()   # contiguous
        whole = HostIndex(self.dim, self.metric)
        whole.add(np.concatenate([s.rows for s in shards]))
        return whole

    def search(self, queries, k):
        return self._whole().search(queries, k)

    def search_subset(self, queries, k, row_ids):
        FakeSharded.log.append(("search_subset", k, len(row_ids)))
        return self._whole().search_subset(queries, k, row_ids)

    def search_collapsed(self, queries, k, cap, keys, fetch_k=None, max_fetch=1024):
        FakeSharded.log.append(("search_collapsed", k, cap, fetch_k, keys.length))
        return self._whole().search_collapsed(queries, k, cap, keys, fetch_k, max_fetch)

    def close(self):
        FakeSharded.alive.remove(self)


def test_per_source_under_a_world_goes_through_the_sharded_searcher(env, monkeypatch):
    import autorag_research_amd.sharded as sharded
    import autorag_research_amd.service as svc

    plain, e = env
    monkeypatch.setattr(sharded, "ShardedSearcher", FakeSharded)
    FakeSharded.alive, FakeSharded.log = [], []
    ranks = []
    for r in range(2):
        s = svc.Mi355RetrievalService(plain.session_factory)
        s._unit("chunk")
        s._world = FakeWorld(r, 2)
        s._unit("chunk").single_searcher(s._world)        # (built lazily: every rank's share must exist before one searches)
        ranks.append(s)
    so = e["source_of"]
    try:
        want = plain.vector_search(["q0", "q1", "q2"], 6, per_source=1, source_of=so, source_fetch_k=12)
        within = [pk for i, pk in enumerate(e["ids"]) if i % 3 != 1]
        want_w = plain.vector_search(["q0", "q1", "q2"], 5, within=within, per_source=1, source_of=so, source_fetch_k=24)
        assert want != plain.vector_search(["q0", "q1", "q2"], 6)
        n_rows = e["n"] - len(e["nulls"])
        for s in ranks:
            assert s.vector_search(["q0", "q1", "q2"], 6, per_source=1, source_of=so, source_fetch_k=12) == want
            assert s.vector_search(["q0", "q1", "q2"], 5, within=within, per_source=1, source_of=so, source_fetch_k=24) == want_w
            u = s._unit("chunk")
            assert u.single is None and u.single_sharded is not None            # nothing local: the searcher's index is the handle
            have = u._source_keys["single"]
            assert have.handle is u.single_sharded.index and have.length == n_rows
            # the table covers the GLOBAL rows (every chunk with an embedding), not this rank's share, and equals the plain one
            assert len(u.single_sharded.rows) < n_rows
            assert np.array_equal(HostIndex.memory[have.ptr], HostIndex.memory[plain._unit("chunk")._source_keys["single"].ptr])
        assert ("search_collapsed", 6, 1, 12, n_rows) in FakeSharded.log and any(c[0] == "search_subset" and c[1] == 24 for c in FakeSharded.log)
        n_up = len(HostIndex.uploads)                                            # once per mapping, under a world too
        ranks[0].vector_search(["q1"], 6, per_source=2, source_of=so)
        assert len(HostIndex.uploads) == n_up
    finally:
        for s in ranks:
            s._world = None
            s.close()
    assert FakeSharded.alive == []
