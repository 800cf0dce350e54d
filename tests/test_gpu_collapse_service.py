"""GPU: the service's `per_source` over the real index -- single mode (with and without `within`), MaxSim and BM25 over a small
table with chunks that have no embedding -- each against the walk applied to the SAME service call without `per_source` at the
depth the capped call searched; and the index's `search_maxsim_collapsed` / `search_bm25_collapsed` convenience methods."""

import numpy as np
import pytest

import collapse_ref as cr

pytestmark = pytest.mark.gpu


def _capped(results, source_of, cap, k):
    seen, out = {}, []
    for r in results:
        src = source_of.get(r["doc_id"])
        if src is not None:
            seen[src] = seen.get(src, 0) + 1
            if seen[src] > cap:
                continue
        out.append(r)
    return out[:k]


WORDS = ["alpha", "beta", "gamma", "delta", "kappa", "sigma", "omega", "theta"]


@pytest.fixture(scope="module")
def env(native_built):
    from autorag_research_amd.service import Mi355RetrievalService
    from autorag_research_amd.store import InMemoryStore

    rng = np.random.default_rng(21)
    n, d, dm = 240, 64, 32
    C = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((3, d)).astype(np.float32)
    C[60:90] = Q[0] + 0.05 * rng.standard_normal((30, d)).astype(np.float32)     # one heavy source in front of query 0
    nulls = [0, 5, 61, 62, 200]
    C[nulls] = np.nan                                                             # index rows are not table positions
    docs = [rng.standard_normal((int(t), dm)).astype(np.float32) for t in rng.integers(2, 7, size=n)]
    docs[3] = None
    contents = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 9)))) for _ in range(n)]
    ids = [f"c{i:03d}" for i in range(n)]
    store = InMemoryStore()
    store.set_chunks(ids, contents, embedding=C, multivec=docs)
    Qm = [rng.standard_normal((t, dm)).astype(np.float32) for t in (3, 5, 2)]
    store.add_queries(["q0", "q1", "q2"], contents=["alpha beta", "gamma delta omega", "theta"], embedding=list(Q), embeddings=Qm)
    source_of = {pk: i // 30 for i, pk in enumerate(ids) if i % 11 != 10}         # sources of 30 chunks; some chunks have none
    s = Mi355RetrievalService(lambda: store)
    yield s, dict(ids=ids, Q=Q, n=n, nulls=nulls, source_of=source_of)
    s.close()


def test_single_mode_deepens_past_the_heavy_source(env):
    s, e = env
    so = e["source_of"]
    full = s.vector_search(["q0", "q1", "q2"], e["n"])                            # every chunk with an embedding, ranked
    assert all(len(f) == e["n"] - len(e["nulls"]) for f in full)
    assert sum(so.get(r["doc_id"]) == 2 for r in full[0][:28]) >= 25              # not vacuous: source 2 fills query 0's head
    for cap in (1, 2):
        for fetch in (None, 6, 64):
            got = s.vector_search(["q0", "q1", "q2"], 6, per_source=cap, source_of=so, source_fetch_k=fetch)
            assert got == [_capped(f, so, cap, 6) for f in full], (cap, fetch)
    one = s.vector_search_by_embedding([float(x) for x in e["Q"][0]], 6, per_source=1, source_of=so)
    assert one == _capped(full[0], so, 1, 6)
    u = s._unit("chunk")
    assert u.single.stat("collapse_researched") > 0 and u.single.stat("collapse_searches") >= 7
    # the key table is the index's rows, not the table's positions
    assert u._source_keys["single"].length == e["n"] - len(e["nulls"])


def test_single_mode_within(env):
    s, e = env
    so = e["source_of"]
    within = [pk for i, pk in enumerate(e["ids"]) if i % 4 != 3] + ["unknown"]
    for depth in (12, 40):
        base = s.vector_search(["q0", "q1"], depth, within=within)
        got = s.vector_search(["q0", "q1"], 5, within=within, per_source=1, source_of=so, source_fetch_k=depth)
        assert got == [_capped(b, so, 1, 5) for b in base]
    assert len(got[0]) == 5 and len(s.vector_search(["q0"], 5, within=within, per_source=1, source_of=so, source_fetch_k=12)[0]) < 5


def test_maxsim_and_bm25(env):
    s, e = env
    so = e["source_of"]
    base = s.vector_search(["q0", "q1", "q2"], 48, "multi")
    got = s.vector_search(["q0", "q1", "q2"], 6, "multi", per_source=1, source_of=so, source_fetch_k=48)
    assert got == [_capped(b, so, 1, 6) for b in base] and any(g != b[:6] for g, b in zip(got, base))
    within = e["ids"][::2]
    base_w = s.maxsim_search_by_embeddings([e["Q"][:1].reshape(2, 32)], 30, within=within)
    got_w = s.maxsim_search_by_embeddings([e["Q"][:1].reshape(2, 32)], 4, within=within, per_source=2, source_of=so, source_fetch_k=30)
    assert got_w == [_capped(base_w[0], so, 2, 4)]
    # BM25: ids are table positions
    base_b = s.bm25_search(["q0", "q1", "q2"], 60)
    got_b = s.bm25_search(["q0", "q1", "q2"], 5, per_source=1, source_of=so, source_fetch_k=60)
    assert got_b == [_capped(b, so, 1, 5) for b in base_b] and any(g != b[:5] for g, b in zip(got_b, base_b))
    text = s.bm25_search_by_text("alpha omega", 4, per_source=2, source_of=so)
    assert text == _capped(s.bm25_search_by_text("alpha omega", s._source_depth(4, None)), so, 2, 4) and s._source_depth(4, None) > 4
    got_bw = s.bm25_search(["q1"], 3, within=within, per_source=1, source_of=so, source_fetch_k=20)
    assert got_bw == [_capped(s.bm25_search(["q1"], 20, within=within)[0], so, 1, 3)]
    with pytest.raises(ValueError):
        s.vector_search(["q0"], 5, per_source=1, source_of=so, mmr_fetch_k=20)


def test_index_convenience_methods(native_built):
    import autorag_research_amd as pkg

    rng = np.random.default_rng(4)
    n, dm = 120, 32
    docs = [rng.standard_normal((int(t), dm)).astype(np.float32) for t in rng.integers(2, 6, size=n)]
    off = np.concatenate([[0], np.cumsum([x.shape[0] for x in docs])]).astype(np.int64)
    qtok = rng.standard_normal((7, dm)).astype(np.float32)
    qoff = np.array([0, 3, 7], dtype=np.int32)
    keys = (np.arange(n) // 10).astype(np.int64)
    keys[::13] = -1
    with pkg.Mi355Index(dm) as ix:
        ix.add_multivec(np.concatenate(docs), off)
        d32, r = ix.search_maxsim(qtok, qoff, 50)
        exp = cr.collapse(d32.astype(np.float64), r, keys, 1, 8)
        dist, ids, k, count = ix.search_maxsim_collapsed(qtok, qoff, 8, 1, keys, 50)
        assert dist.dtype == np.float32 and np.array_equal(ids, exp.ids) and np.array_equal(k, exp.keys)
        assert np.array_equal(count, exp.count)
        want = np.where(exp.pos >= 0, np.take_along_axis(d32, np.maximum(exp.pos, 0), axis=1), np.float32(np.nan))
        assert np.array_equal(dist.view(np.uint32), want.view(np.uint32)) and (exp.pos[:, :8] >= 0).all()   # the search's own bits
        toks = [list(rng.integers(0, 40, size=int(t))) for t in rng.integers(3, 12, size=n)]
        ix.add_sparse(toks)
        queries = [[1, 2, 3], [7, 30]]
        bd, br = ix.search_bm25(queries, 40)
        expb = cr.collapse(bd, br, keys, 2, 6)
        with ix.upload_keys(keys) as table:
            for t in (keys, table):
                dist, ids, k, count = ix.search_bm25_collapsed(queries, 6, 2, t, 40)
                assert np.array_equal(dist.view(np.uint64), expb.vals.view(np.uint64)) and np.array_equal(ids, expb.ids)
                assert np.array_equal(k, expb.keys) and np.array_equal(count, expb.count)
