"""GPU: search within a listed subset of rows (mi355dr_search_subset / _device, mi355dr_score_subset) against the CPU oracle,
bit for bit in ids and float8 distances (NaN positions must match, NaN payloads are not part of the contract).

Oracle of the restricted search: with the listed rows sorted and unique, `topk_search(C[ids], Q, k, metric)` with rows mapped
back through `ids`.  Sorted ids keep positions in id order, so position order is row order and the tie rule carries over: it
is the full oracle ranking filtered to the listed rows."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = [1, 10, 32, 33, 128, 129, 1024]      # the prune forms' edges and kKMax
N_SMALL = 4099                            # 16 workgroups of 256 positions and a last group of 3 rows


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def _same(a, b):
    """two (dist, rows) results agree bit for bit (NaN positions, not payloads)"""
    (da, ra), (db, rb) = a, b
    assert np.array_equal(ra, rb)
    assert np.array_equal(np.isnan(da), np.isnan(db))
    ok = ~np.isnan(da)
    assert np.array_equal(da[ok].view(np.uint64), db[ok].view(np.uint64))


def expect(oracle, C, Q, k, ids, metric="cosine", row_offset=0, live=None):
    """the oracle's answer for the GLOBAL ids `ids` over the corpus C (rows not in `live`, when given, are removed)"""
    ids = np.unique(np.asarray(ids, dtype=np.int64).reshape(-1) - row_offset)
    ids = ids[(ids >= 0) & (ids < C.shape[0])]
    if live is not None:
        ids = ids[live[ids]]
    d, r = oracle.topk_search(C[ids], Q, k, metric=metric)
    return d, np.where(r >= 0, (ids[np.maximum(r, 0)] if ids.size else 0) + row_offset, -1)


_CORPORA = {}


def corpus(d, n=N_SMALL, B=40):
    if (d, n, B) not in _CORPORA:
        rng = np.random.default_rng([d, n, B])
        _CORPORA[(d, n, B)] = (rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((B, d)).astype(np.float32))
    return _CORPORA[(d, n, B)]


@pytest.mark.parametrize("metric", ["cosine", "ip"])
@pytest.mark.parametrize("d", [128, 100, 50], ids=["d128", "d100-vector-staging", "d50-scalar-staging"])
def test_dims_metrics_k_and_query_groups(pkg, oracle, d, metric):
    """rows that are whole 128-byte pieces, rows staged as float4 and rows staged scalar; one query group (B = 24) and two
    with the second partial (B = 40); every k in KS over a list of 1501 rows (a second, list-sized chunk behind the first
    1024 positions, a last wave of 29), and k above the 37 rows of a short list (NaN / -1 tail)"""
    C, Q = corpus(d)
    rng = np.random.default_rng(d)
    ids = rng.choice(N_SMALL, size=1501, replace=False)
    short = rng.choice(N_SMALL, size=37, replace=False)
    with pkg.Mi355Index(d, metric) as idx:
        idx.add(C)
        for B in (24, 40):
            for k in KS:
                _same(idx.search_subset(Q[:B], k, ids), expect(oracle, C, Q[:B], k, ids, metric))
            got = idx.search_subset(Q[:B], 50, short)
            _same(got, expect(oracle, C, Q[:B], 50, short, metric))
            assert (got[1][:, 37:] == -1).all() and (got[1][:, :37] >= 0).all()
        assert idx.stat("subset_searches") == 2 * (len(KS) + 1)
        assert idx.stat("subset_rows_scored") == (24 + 40) * (len(KS) * 1501 + 37)
        assert idx.stat("screen_launches") == 0 and idx.stat("subset_rerun_queries") == 0


# ---- the overflow re-run: a chunk of the position ladder larger than the 2048-slot list, on rows sorted by rising similarity
N_ASC, D_ASC, B_ASC = 29_696, 128, 24


def ascending_case():
    """rows sorted by RISING similarity to q0 (every row enters the running top-k of the queries near q0); the queries share
    that direction: q0, 3 q0, q0 plus noise of four sizes, -q0 (the reversed order), and random ones"""
    if "asc" not in _CORPORA:
        rng = np.random.default_rng(2024)
        q0 = rng.standard_normal(D_ASC).astype(np.float32)
        C = rng.standard_normal((N_ASC, D_ASC)).astype(np.float32)
        s = (C.astype(np.float64) @ q0.astype(np.float64)) / np.linalg.norm(C.astype(np.float64), axis=1)
        C = C[np.argsort(s, kind="stable")]
        Q = rng.standard_normal((B_ASC, D_ASC)).astype(np.float32)
        Q[0], Q[1], Q[6] = q0, 3.0 * q0, -q0
        for i, eps in enumerate((1e-3, 1e-2, 5e-2, 0.2)):
            Q[2 + i] = q0 + eps * rng.standard_normal(D_ASC).astype(np.float32)
        _CORPORA["asc"] = (C, Q)
    return _CORPORA["asc"]


@pytest.mark.parametrize("k", [10, 100])
def test_overflowed_chunk_is_rerun_in_pieces(pkg, oracle, k):
    """list = every second row, m = 14 848: behind the first 1024 positions the ladder's second chunk (13 824 positions) is
    larger than the list and overflows it for the queries near q0, which take the re-run in list-sized pieces"""
    C, Q = ascending_case()
    ids = np.arange(0, N_ASC, 2)
    with pkg.Mi355Index(D_ASC) as idx:
        idx.add(C)
        _same(idx.search_subset(Q, k, ids), expect(oracle, C, Q, k, ids))
        rerun = idx.stat("subset_rerun_queries")
        print(f"k={k}: {rerun} of {B_ASC} queries re-run in pieces")
        # q0 and 3 q0 see (nearly) every row of the chunk enter their top-k: 13 824 appends into 2048 slots; -q0 sees the best
        # rows first and the random queries append ~ k ln(ratio) rows: no overflow for them
        assert 2 <= rerun < B_ASC
        assert idx.stat("fallback_queries") == 0 and idx.stat("screen_launches") == 0


def test_list_hygiene_and_row_offset(pkg, oracle):
    """shuffled, with duplicates, with -1 padding and with ids outside the index mixed in: the answer of the clean sorted list;
    with row_offset = 1000 listed ids and returned rows are global"""
    C, Q = corpus(100)
    rng = np.random.default_rng(5)
    clean = np.sort(rng.choice(N_SMALL, size=900, replace=False))
    for off in (0, 1000):
        dirty = np.concatenate([clean + off, (clean + off)[::7], np.full(50, -1),
                                [-5, off - 1, N_SMALL + off, N_SMALL + off + 1, 2**40, -2**40]])
        rng.shuffle(dirty)
        with pkg.Mi355Index(100) as idx:
            idx.set_option("row_offset", off)
            idx.add(C)
            want = expect(oracle, C, Q, 33, clean + off, row_offset=off)
            assert want[1].min() >= off
            _same(idx.search_subset(Q, 33, clean + off), want)
            _same(idx.search_subset(Q, 33, dirty), want)
            if off:   # ids below row_offset and at or above row_offset + size belong to other shards
                low_high = np.concatenate([clean + off, np.arange(0, off, 3), np.arange(N_SMALL + off, N_SMALL + off + 40)])
                _same(idx.search_subset(Q, 33, low_high), want)
                assert idx.search_subset(Q[:2], 3, np.arange(0, off))[1].max() == -1


def test_row_classes(pkg, oracle):
    """removed rows (before and after compact, the list rewritten through new_of_old), updated rows, irregular rows (0 / NaN /
    +-inf: last, with NaN) and more than k exact duplicates (tie order by row)"""
    d, n = 100, 3000
    C, Q = corpus(d, n, 24)
    C, Q = C.copy(), Q.copy()
    rng = np.random.default_rng(8)
    ids = np.sort(rng.choice(n, size=700, replace=False))
    for v, r in zip((0.0, np.nan, np.inf, -np.inf, 0.0), ids[[3, 90, 91, 400, 699]]):
        C[r] = v
    dup = ids[100:160:2]                                  # 30 listed copies of a row near Q[0] ...
    C[dup] = Q[0] + 0.01 * rng.standard_normal(d).astype(np.float32)
    unlisted = np.setdiff1d(np.arange(n), ids)
    C[unlisted[unlisted > dup[0]][0]] = C[dup[0]]         # ... and an unlisted one between them, which must not show up
    shuffled = rng.permutation(ids)
    with pkg.Mi355Index(d) as idx:
        idx.add(C)
        for k in (10, 129, 1024):
            got = idx.search_subset(Q, k, shuffled)
            _same(got, expect(oracle, C, Q, k, ids))
        assert got[1][0, :30].tolist() == dup.tolist()                      # the ties, in row order
        assert np.isnan(got[0][:, 695:700]).all() and (got[1][:, 695:700] >= 0).all() and (got[1][:, 700:] == -1).all()
        live = np.ones(n, bool)
        gone = np.concatenate([ids[5:300:3], dup[:4], rng.choice(n, size=200, replace=False)])
        gone = np.unique(gone)
        idx.remove_rows(gone)
        live[gone] = False
        for k in (10, 129, 1024):
            _same(idx.search_subset(Q, k, shuffled), expect(oracle, C, Q, k, ids, live=live))
        changed = np.unique(np.concatenate([ids[301:330], gone[:20]]))      # updated rows, some of them revived
        C[changed] = rng.standard_normal((changed.size, d)).astype(np.float32)
        idx.update_rows(changed, C[changed])
        live[changed] = True
        for k in (10, 129):
            _same(idx.search_subset(Q, k, shuffled), expect(oracle, C, Q, k, ids, live=live))
        new_of_old = idx.compact()
        C2, moved = C[live], new_of_old[shuffled]                           # (-1 for a removed row: skipped)
        assert (moved == -1).sum() == (~live[ids]).sum() > 0
        for k in (10, 129, 1024):
            _same(idx.search_subset(Q, k, moved), expect(oracle, C2, Q, k, moved))


def test_edges(pkg, oracle):
    """no list, one row, every row (= the scan path, bit for bit), and a list inside the last, partial 64-row group"""
    C, Q = corpus(128)
    with pkg.Mi355Index(128) as idx:
        idx.add(C)
        d0, r0 = idx.search_subset(Q, 5, np.zeros(0, np.int64))
        assert np.isnan(d0).all() and (r0 == -1).all()
        _same(idx.search_subset(Q, 5, [N_SMALL - 1]), expect(oracle, C, Q, 5, [N_SMALL - 1]))
        _same(idx.search_subset(Q, 1, [0]), expect(oracle, C, Q, 1, [0]))
        tail = np.arange(4096, N_SMALL)
        _same(idx.search_subset(Q, 10, tail), expect(oracle, C, Q, 10, tail))
        every = idx.search_subset(Q, 100, np.arange(N_SMALL))
        idx.set_option("path", "scan")
        _same(every, idx.search(Q, 100))
        _same(every, oracle.topk_search(C, Q, 100))
        # bad shapes
        from autorag_research_amd._native import NativeError

        with pytest.raises(NativeError):
            idx.search_subset(Q, 0, tail)
        with pytest.raises(NativeError):
            idx.search_subset(Q, 1025, tail)
        with pytest.raises(ValueError):
            idx.search_subset(Q, 5, np.zeros((2, 2), np.int64))


def test_device_entry_and_state(pkg, oracle):
    """device buffers in and out match the host entry; a normal search before and after is unchanged (the per-search state
    is left clean); a subset call that arrives while an async block is in flight completes that block first"""
    C, Q = corpus(128)
    k, ids = 33, np.arange(1, N_SMALL, 3)
    with pkg.Mi355Index(128) as idx:
        idx.add(C)
        full = idx.search(Q, k)
        _same(full, oracle.topk_search(C, Q, k))
        host = idx.search_subset(Q, k, ids)
        _same(host, expect(oracle, C, Q, k, ids))
        pq, od, orr = idx.dev_alloc(Q.nbytes), idx.dev_alloc(len(Q) * k * 8), idx.dev_alloc(len(Q) * k * 8)
        od2, or2 = idx.dev_alloc(len(Q) * k * 8), idx.dev_alloc(len(Q) * k * 8)
        idx.dev_upload(pq, Q)
        ticket = idx.search_device_async(pq, len(Q), k, od2, or2)          # in flight ...
        idx.search_subset_device(pq, len(Q), k, ids, od, orr)              # ... when the subset call arrives
        gd, gr = np.empty((len(Q), k)), np.empty((len(Q), k), dtype=np.int64)
        idx.dev_download(od, gd)
        idx.dev_download(orr, gr)
        _same((gd, gr), host)
        idx.search_wait(ticket)
        idx.dev_download(od2, gd)
        idx.dev_download(or2, gr)
        _same((gd, gr), full)
        _same(idx.search(Q, k), full)
        _same(idx.search(Q, 100), oracle.topk_search(C, Q, 100))           # a two-wave-prune pass behind a 2048-slot pass
        _same(idx.search_subset(Q, 100, ids), expect(oracle, C, Q, 100, ids))
        for p in (pq, od, orr, od2, or2):
            idx.dev_free(p)


@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_score_subset(pkg, oracle, metric):
    """[B, m] per-query lists, shuffled, with padding, removed rows and out-of-range ids: every finite entry has the oracle's
    bits, NaN exactly at skipped ids, removed rows and undefined distances"""
    d, n, B, m = 50, 700, 9, 41
    C, Q = corpus(d, n, B)
    C = C.copy()
    C[11] = 0.0
    rng = np.random.default_rng(3)
    cand = rng.integers(0, n, size=(B, m))
    off = 500
    cand[:, 5], cand[:, 6], cand[:, 7], cand[2, 8:12] = -1, n + off, 11, (-7, n + off + 9, 2**35, 600)
    gone = np.array([600, 601, 17])
    cand[3, :3] = gone
    with pkg.Mi355Index(d, metric) as idx:
        idx.set_option("row_offset", off)
        idx.add(C)
        idx.remove_rows(gone)
        got = idx.score_subset(Q, np.where((cand >= 0) & (cand < n), cand + off, cand))
    want = np.full((B, m), np.nan)
    for b in range(B):
        dd, rr = oracle.topk_search(C, Q[b], n, metric=metric)
        by_row = np.full(n, np.nan)
        by_row[rr[0]] = dd[0]
        if metric == "cosine":
            assert by_row[3] == oracle.cosine_distance(Q[b], C[3])
        by_row[gone] = np.nan
        ok = (cand[b] >= 0) & (cand[b] < n)
        want[b, ok] = by_row[cand[b, ok]]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(want[:, 5:7]).all() and np.isnan(want[3, :3]).all() and np.isnan(want[:, 7]).all() == (metric == "cosine")
    fin = ~np.isnan(want)
    assert fin.sum() > B * (m - 8) and np.array_equal(got[fin].view(np.uint64), want[fin].view(np.uint64))


def test_service_within_and_score_candidates(pkg, oracle):
    """the service over a small ChunkTable: `within=` and `score_candidates` against the oracle through the table's keys;
    unknown keys and NULL embeddings are ignored"""
    from autorag_research_amd.service import Mi355RetrievalService
    from autorag_research_amd.store import InMemoryStore

    rng = np.random.default_rng(12)
    n, d = 300, 64
    C = rng.standard_normal((n, d)).astype(np.float32)
    nulls = [0, 7, 8, 150, 299]
    C[nulls] = np.nan
    keys = [f"c{i:03d}" for i in range(n)]
    store = InMemoryStore()
    store.set_chunks(keys, [f"t{i}" for i in range(n)], embedding=C)
    q = rng.standard_normal(d).astype(np.float32)
    store.add_queries(["q"], contents=["q"], embedding=[q])
    within = [keys[i] for i in rng.choice(n, size=80, replace=False)] + ["nope", keys[7], keys[150], keys[20], keys[20]]
    pos = sorted({keys.index(pk) for pk in within if pk in keys} - set(nulls))
    s = Mi355RetrievalService(lambda: store)
    try:
        for k in (5, 200):
            dd, rr = oracle.topk_search(C[pos], q, k)
            want = [(keys[pos[j]], 1.0 - float(x)) for x, j in zip(dd[0], rr[0]) if j >= 0]
            got = s.vector_search_by_embedding([float(x) for x in q], k, within=within)
            assert [(r["doc_id"], r["score"]) for r in got] == want
            assert [(r["doc_id"], r["score"]) for r in s.vector_search(["q"], k, within=within)[0]] == want
        sc = s.score_candidates([float(x) for x in q], within)
        assert sorted(sc) == [keys[p] for p in pos]
        assert all(v == 1.0 - oracle.cosine_distance(q, C[keys.index(pk)]) for pk, v in sc.items())
        assert s.vector_search_by_embedding([float(x) for x in q], 5, within=["nope", keys[0]]) == []
        assert len(s.vector_search_by_embedding([float(x) for x in q], 5)) == 5
    finally:
        s.close()


def test_sharded_pipeline_at_world_one(pkg, oracle, tmp_path):
    """ShardedSearcher with force_pipeline at world 1: pack, all-gather, host merge -- the plain index's result"""
    import torch.distributed as dist

    from autorag_research_amd.sharded import ShardedSearcher

    C, Q = corpus(100)
    ids = np.arange(2, N_SMALL, 5) + 700
    cand = np.tile(ids[:30], (len(Q), 1))
    cand[:, 3] = 5                                        # below the shard's first row
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'pg'}", rank=0, world_size=1)
    try:
        s = ShardedSearcher(100, "cosine", device=0)
        s.force_pipeline = True
        s.add_local(C, 700)
        want = expect(oracle, C, Q, 12, ids, row_offset=700)
        _same(s.search_subset(Q, 12, ids), want)
        _same(s.search_subset(Q, 12, ids, block=16), want)
        _same(s.index.search_subset(Q, 12, ids), want)
        sc = s.score_subset(Q, cand)
        plain = s.index.score_subset(Q, cand)
        assert np.isnan(sc[:, 3]).all() and np.array_equal(np.isnan(sc), np.isnan(plain))
        assert np.array_equal(sc[~np.isnan(sc)].view(np.uint64), plain[~np.isnan(plain)].view(np.uint64))
        assert sc[0, 0] == oracle.cosine_distance(Q[0], C[ids[0] - 700])
        s.close()
    finally:
        dist.destroy_process_group()
