"""CPU: MMR search -- the reference itself (tests/mmr_ref.py) and the service's `mmr_fetch_k` / `mmr_lambda` keyword
arguments over an oracle-backed index that answers `search_mmr` / `mmr_select` through that reference."""

import numpy as np
import pytest

import mmr_ref
from helpers import OracleIndex


class OracleMmrIndex(OracleIndex):
    """OracleIndex + the listed-subset search and the two MMR entry points of Mi355Index (global ids)."""

    calls: list = []

    def search_subset(self, queries, k, row_ids):
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        ids = np.unique(np.asarray(row_ids, dtype=np.int64).reshape(-1) - self.row_offset)
        ids = ids[(ids >= 0) & (ids < len(self))]
        d, r = self._o.topk_search(self._rows[ids], q, k, metric=self.metric)
        return d, np.where(r >= 0, ids[np.maximum(r, 0)] + self.row_offset if ids.size else -1, -1)

    def search_mmr(self, queries, k, fetch_k, lambda_mult=0.5):
        self.calls.append(("search_mmr", k, fetch_k, lambda_mult))
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        return mmr_ref.search_mmr(self._o, self._rows, q, k, fetch_k, lambda_mult, self.metric, self.row_offset)[:2]

    def mmr_select(self, queries, k, cand_rows, lambda_mult=0.5):
        self.calls.append(("mmr_select", k, np.asarray(cand_rows).shape[1], lambda_mult))
        return mmr_ref.mmr_select(self._o, self._rows, queries, k, cand_rows, lambda_mult, self.metric, self.row_offset)[:2]


# ---- the reference --------------------------------------------------------------------------------------------------------
def test_reference_by_hand(oracle):
    """three rows, one query along the first two (exact duplicates): lambda = 1 keeps the search's order; lambda = 0.4 takes
    the distinct row second (0.4 * 0.6 - 0.6 * 0.6 = -0.12 against 0.4 * 1 - 0.6 * 1 = -0.2); lambda = 0.5 ties them at 0 and
    the earlier candidate wins; k above the eligible candidates leaves a NaN / -1 tail and the zero row is never picked"""
    C = np.array([[1, 0], [1, 0], [0.6, 0.8], [0, 0]], dtype=np.float32)
    q = np.array([[1, 0]], dtype=np.float32)
    for lam, want in ((1.0, [0, 1, 2]), (0.4, [0, 2, 1]), (0.5, [0, 1, 2]), (0.0, [0, 2, 1])):
        d, r, pairs = mmr_ref.search_mmr(oracle, C, q, 5, 4, lam)
        assert r[0].tolist() == want + [-1, -1] and np.isnan(d[0, 3:]).all() and pairs == 2 + 1
        assert d[0, 0] == 0.0 and d[0, want.index(2)] == oracle.cosine_distance(q[0], C[2])
    d, r, pairs = mmr_ref.search_mmr(oracle, C, q, 1, 4, 0.0)
    assert r.tolist() == [[0]] and pairs == 0
    d, r, _ = mmr_ref.search_mmr(oracle, C, q, 3, 4, 0.4, metric="ip")     # ip: the zero row is an ordinary candidate
    assert r[0].tolist() == [0, 3, 2]                                       # -0.6 * 0 > 0.4 * 0.6 - 0.6 * 0.6 > 0.4 - 0.6


@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_reference_pair_distances_and_lambda_one(oracle, metric):
    """one oracle call per pair (the definition) and one `topk_search` per picked row give the same picks; lambda = 1 is the
    plain top-k for every query; at lambda = 0.5 every query of both corpora leaves it (the GPU tests discriminate)"""
    for C, Q in (mmr_ref.clustered(32, 12), mmr_ref.gaussian(32, 12)):
        plain = oracle.topk_search(C, Q, 10, metric=metric)
        mmr_ref.same(mmr_ref.search_mmr(oracle, C, Q, 10, 32, 1.0, metric), plain)
        half = mmr_ref.search_mmr(oracle, C, Q, 10, 32, 0.5, metric)
        slow = mmr_ref.search_mmr(oracle, C, Q[:3], 10, 32, 0.5, metric, pairdist=mmr_ref.pairdist_scalar)
        mmr_ref.same((half[0][:3], half[1][:3]), slow)
        assert (half[1] != plain[1]).any(axis=1).all()
        assert (half[1][:, 0] == plain[1][:, 0]).all()                     # pick 0 is the nearest row
        assert all(set(a) <= set(b) for a, b in zip(half[1].tolist(), oracle.topk_search(C, Q, 32, metric=metric)[1].tolist()))


def test_reference_select_hygiene(oracle):
    C, Q = mmr_ref.gaussian(32, 3)
    pool = np.array([[5, 900, -1, 5, 2000, 77, 1999, -7], [1, 2, 3, 4, 5, 6, 7, 8], [-1] * 8])
    live = np.ones(2000, dtype=bool)
    live[900] = False
    d, r, _ = mmr_ref.mmr_select(oracle, C, Q, 4, pool, 0.5, live=live)
    assert sorted(r[0].tolist()) == [-1, 5, 77, 1999] and (r[2] == -1).all() and np.isnan(d[2]).all()
    mmr_ref.same(mmr_ref.mmr_select(oracle, C, Q[1:2], 4, pool[1:2], 1.0), oracle_subset(oracle, C, Q[1:2], 4, pool[1]))
    d, r, pairs = mmr_ref.mmr_select(oracle, C, Q, 3, np.zeros((3, 0), dtype=np.int64), 0.5)
    assert (r == -1).all() and pairs == 0


def oracle_subset(oracle, C, Q, k, ids):
    ids = np.unique(np.asarray(ids, dtype=np.int64))
    d, r = oracle.topk_search(C[ids], Q, k)
    return d, np.where(r >= 0, ids[np.maximum(r, 0)], -1)


# ---- the service's keyword arguments ----------------------------------------------------------------------------------------
@pytest.fixture()
def svc_env(monkeypatch, oracle):
    import autorag_research_amd.service as svc
    from autorag_research_amd.store import InMemoryStore

    monkeypatch.setattr(svc, "Mi355Index", OracleMmrIndex)
    monkeypatch.setattr(OracleMmrIndex, "calls", [])
    rng = np.random.default_rng(41)
    n, d = 120, 24
    centres = rng.standard_normal((12, d))
    C = (np.repeat(centres, 10, axis=0) + 0.05 * rng.standard_normal((n, d))).astype(np.float32)
    nulls = [0, 13, 55]
    C[nulls] = np.nan                                   # NULL embedding
    ids = [f"c{i:03d}" for i in range(n)]
    store = InMemoryStore()
    store.set_chunks(ids, [f"text {i}" for i in range(n)], embedding=C,
                     multivec=[rng.standard_normal((2, 8)).astype(np.float32) for _ in range(n)])
    Q = (centres[[3, 7, 3]] + 0.3 * rng.standard_normal((3, d))).astype(np.float32)
    store.add_queries(["q0", "q1", "q2"], contents=["a", "b", "c"], embedding=list(Q),
                      embeddings=[rng.standard_normal((2, 8)).astype(np.float32) for _ in range(3)])
    return svc.Mi355RetrievalService(lambda: store), dict(C=C, ids=ids, nulls=nulls, Q=Q)


def _expected(oracle, e, q, keys, k, fetch_k, lam):
    """MMR over the oracle ranking of the listed keys that have an embedding: [(key, score)] in selection order"""
    pos = sorted({e["ids"].index(pk) for pk in keys if pk in e["ids"]} - set(e["nulls"]))
    d, r, _ = mmr_ref.search_mmr(oracle, e["C"][pos], q, k, fetch_k, lam)
    return [(e["ids"][pos[j]], 1.0 - float(x)) for x, j in zip(d[0], r[0]) if j >= 0]


def _pairs(results):
    return [(r["doc_id"], r["score"]) for r in results]


def test_service_none_is_todays_behaviour(svc_env):
    s, e = svc_env
    emb = [float(x) for x in e["Q"][1]]
    keys = ["c030", "c031", "c077", "nope", "c013"]
    assert s.vector_search(["q0", "q1"], 7) == s.vector_search(["q0", "q1"], 7, mmr_fetch_k=None, mmr_lambda=0.1)
    assert s.vector_search_by_embedding(emb, 7) == s.vector_search_by_embedding(emb, 7, mmr_fetch_k=None)
    assert s.vector_search_by_embedding(emb, 3, within=keys) == s.vector_search_by_embedding(emb, 3, within=keys, mmr_fetch_k=None)
    assert s.vector_search(["q2"], 3, "multi") == s.vector_search(["q2"], 3, "multi", mmr_fetch_k=None)
    assert OracleMmrIndex.calls == []


def test_service_mmr_without_within(svc_env, oracle):
    s, e = svc_env
    blocks = s.vector_search(["q0", "q1", "q2"], 6, "single", mmr_fetch_k=20, mmr_lambda=0.5)
    plain = s.vector_search(["q0", "q1", "q2"], 6, "single")
    for b, got in enumerate(blocks):
        assert _pairs(got) == _expected(oracle, e, e["Q"][b], e["ids"], 6, 20, 0.5)
        assert [r["doc_id"] for r in got] != [r["doc_id"] for r in plain[b]] and got[0] == plain[b][0]
        assert all(r["content"] == f"text {int(r['doc_id'][1:])}" for r in got)
    one = s.vector_search_by_embedding([float(x) for x in e["Q"][1]], 6, mmr_fetch_k=20, mmr_lambda=0.3)
    assert _pairs(one) == _expected(oracle, e, e["Q"][1], e["ids"], 6, 20, 0.3)
    assert _pairs(s.vector_search_by_embedding([float(x) for x in e["Q"][1]], 6, mmr_fetch_k=20, mmr_lambda=1.0)) == _pairs(plain[1])
    assert s.vector_search_by_embedding([], 6, mmr_fetch_k=20) == []
    assert OracleMmrIndex.calls == [("search_mmr", 6, 20, 0.5), ("search_mmr", 6, 20, 0.3), ("search_mmr", 6, 20, 1.0)]


def test_service_mmr_within(svc_env, oracle):
    s, e = svc_env
    keys = [f"c{i:03d}" for i in list(range(28, 52)) + [13, 55, 30]] + ["nope", 17]     # three clusters, two NULL rows
    for k, fetch_k in ((5, 12), (5, 64)):                                              # a pool cut at 12; the whole list (24 rows)
        got = s.vector_search(["q0", "q1"], k, within=keys, mmr_fetch_k=fetch_k, mmr_lambda=0.5)
        for b, res in enumerate(got):
            assert _pairs(res) == _expected(oracle, e, e["Q"][b], keys, k, fetch_k, 0.5)
    one = s.vector_search_by_embedding([float(x) for x in e["Q"][0]], 30, within=keys, mmr_fetch_k=40, mmr_lambda=0.0)
    assert _pairs(one) == _expected(oracle, e, e["Q"][0], keys, 30, 40, 0.0) and len(one) == 24
    assert s.vector_search_by_embedding([float(x) for x in e["Q"][0]], 5, within=["nope", "c013"], mmr_fetch_k=9) == []
    assert [c[:3] for c in OracleMmrIndex.calls] == [("mmr_select", 5, 12), ("mmr_select", 5, 64), ("mmr_select", 30, 40),
                                                     ("mmr_select", 5, 9)]
    with pytest.raises(ValueError):
        s.vector_search_by_embedding([float(x) for x in e["Q"][0]], 5, within=keys, mmr_fetch_k=4)


def test_service_mmr_refuses_multi_and_a_world(svc_env):
    s, e = svc_env
    with pytest.raises(ValueError):
        s.vector_search(["q0"], 3, "multi", mmr_fetch_k=10)
    s._world = object()          # a process group: refused before anything is asked of it
    with pytest.raises(NotImplementedError):
        s.vector_search(["q0"], 3, mmr_fetch_k=10)
    with pytest.raises(NotImplementedError):
        s.vector_search_by_embedding([float(x) for x in e["Q"][0]], 3, mmr_fetch_k=10)
    with pytest.raises(NotImplementedError):
        s.vector_search_by_embedding([float(x) for x in e["Q"][0]], 3, within=["c001"], mmr_fetch_k=10)
    s._world = None
    assert OracleMmrIndex.calls == []
