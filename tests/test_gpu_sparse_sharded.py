"""GPU, one process: the row-sharded sparse entry points at world size 1 over `mi355dr_comm_init_custom` with a copy-through
transport.  At one rank every sharded form must equal its local form on the same handle bit for bit -- with `row_offset` set,
small tiles, a candidate list small enough to overflow, B across the 1024-query block, and a mutated store (overlay active);
the refusals come before the first collective and leave stats and results alone; the stats move as include/mi355dr.h says."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -4
N_DOCS, VOCAB, OFFSET, B = 3000, 400, 7000, 1100


def _docs():
    rng = np.random.default_rng(41)
    lens = rng.integers(0, 61, size=N_DOCS)
    lens[::97] = 0
    return [rng.integers(0, VOCAB, size=int(n)).tolist() for n in lens]


def _token_queries():
    rng = np.random.default_rng(42)
    qs = [rng.integers(0, VOCAB + 20, size=int(rng.integers(1, 7))).tolist() for _ in range(B)]
    qs[5], qs[1030] = [], [VOCAB + 3, -1, 1 << 21]     # no term; no term that occurs
    return qs


def _weighted_queries(n):
    rng = np.random.default_rng(43)
    terms, weights, off = [], [], [0]
    for j in range(n):
        t = rng.choice(VOCAB + 10, size=int(rng.integers(0, 6)), replace=False)
        terms += t.tolist()
        weights += rng.uniform(-1.0, 2.0, size=len(t)).tolist()
        off.append(len(terms))
    return np.array(terms, dtype=np.int32), np.array(weights), np.array(off, dtype=np.int32)


def _same(a, b):
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape
    assert np.array_equal(np.ascontiguousarray(a[0]).view(np.int64), np.ascontiguousarray(b[0]).view(np.int64))
    assert np.array_equal(a[1], b[1])


def _same_scores(a, b):
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    assert np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64))


def _make(cand_cap=None, docs=None):
    import autorag_research_amd as pkg

    idx = pkg.Mi355Index(8)
    idx.set_option("row_offset", OFFSET)
    idx.set_option("sparse_tile_docs", 256)
    if cand_cap is not None:
        idx.set_option("sparse_subset_pairs_max", 0)
        idx.set_option("sparse_cand_cap", cand_cap)
    idx.add_sparse(_docs() if docs is None else docs)
    calls = []

    def all_gather(send_ptr, recv_ptr, nbytes, stream):
        tmp = np.empty(nbytes // 8, dtype=np.int64)
        idx.dev_download(send_ptr, tmp)
        idx.dev_upload(recv_ptr, tmp)
        calls.append(nbytes)

    idx.comm_init_custom(0, 1, all_gather)
    return idx, calls


@pytest.fixture(scope="module")
def looped(native_built):
    idx, calls = _make()
    yield idx, calls
    idx.close()


@pytest.fixture(scope="module")
def queries():
    return _token_queries(), _weighted_queries(B)


def _every_form(idx, tq, wq, ks):
    rng = np.random.default_rng(44)
    short = np.concatenate([rng.integers(OFFSET, OFFSET + N_DOCS, size=40), [-1, OFFSET - 1, OFFSET + N_DOCS, OFFSET + 5, OFFSET + 5]])
    long_ = rng.integers(OFFSET - 50, OFFSET + N_DOCS + 50, size=900)
    for k in ks:
        _same(idx.search_bm25_sharded(tq, k), idx.search_bm25(tq, k))
        _same(idx.search_sparse_sharded(*wq, k, 0.9, 0.4), idx.search_sparse(*wq, k, 0.9, 0.4))
        for ids in (short, long_):
            _same(idx.search_bm25_subset_sharded(tq, k, ids), idx.search_bm25_subset(tq, k, ids))
            _same(idx.search_sparse_subset_sharded(*wq, k, ids), idx.search_sparse_subset(*wq, k, ids))
    pool = rng.integers(OFFSET - 3, OFFSET + N_DOCS + 3, size=(B, 9))
    pool[:, 4], pool[:, 6] = pool[:, 3], -1
    _same_scores(idx.score_bm25_subset_sharded(tq, pool), idx.score_bm25_subset(tq, pool))
    _same_scores(idx.score_sparse_subset_sharded(*wq, pool, 0.9, 0.4), idx.score_sparse_subset(*wq, pool, 0.9, 0.4))


@pytest.mark.parametrize("k", [1, 10, 100])
def test_every_sharded_form_equals_its_local_form(looped, queries, k):
    idx, calls = looped
    idx.set_option("sparse_subset_pairs_max", 64)       # the short list takes the pair pass, the long one the tile pass
    del calls[:]
    _every_form(idx, *queries, [k])
    assert calls and all(n % 8 == 0 for n in calls)
    hits = idx.search_bm25(queries[0], k)[1]
    assert (hits >= OFFSET).sum() > B // 2 and (hits[5] == -1).all() and (hits[1030] == -1).all()


def test_overflow_pieces_run_under_a_small_candidate_list(native_built, queries):
    idx, calls = _make(cand_cap=16)
    try:
        idx.reset_stats()
        _same(idx.search_bm25_sharded(queries[0], 10), idx.search_bm25(queries[0], 10))
        assert idx.stat("sparse_overflows") > 0
        long_ = np.arange(OFFSET, OFFSET + N_DOCS, 2)
        _same(idx.search_bm25_subset_sharded(queries[0], 10, long_), idx.search_bm25_subset(queries[0], 10, long_))
        assert idx.stat("sparse_subset_tiles") > 0
    finally:
        idx.close()


def test_a_mutated_store_with_its_overlay(native_built, queries):
    idx, calls = _make()
    try:
        tq, wq = queries
        idx.search_bm25(tq[:4], 5)                       # the base layout
        rng = np.random.default_rng(45)
        idx.set_sparse([3, 700, 2999], [[1, 2, 3, 3], [], rng.integers(0, VOCAB, size=50).tolist()])
        idx.remove_sparse([10, 11])
        idx.add_sparse([[7, 8, 9], [], [VOCAB + 1] * 3])
        idx.reset_stats()
        _same(idx.search_bm25_sharded(tq, 10), idx.search_bm25(tq, 10))
        assert idx.stat("sparse_overlay_builds") == 1 and idx.stat("sparse_overlay_postings") > 0
        _every_form(idx, tq, wq, [10])
        # the two kinds of call alternate on one handle: each scores with its own statistics (the same ones at world 1)
        assert idx.stat("sparse_full_builds") == 0
    finally:
        idx.close()


def test_a_store_without_documents_enters_the_collectives(native_built):
    idx, calls = _make(docs=[])
    try:
        d, r = idx.search_bm25_sharded([[1, 2], []], 3)
        assert np.isnan(d).all() and (r == -1).all() and d.shape == (2, 3)
        assert calls == [8 * (2 + 2), 8 * 2 * 2 * 3]     # the statistics [2 + T], one packed block
        assert np.isnan(idx.score_bm25_subset_sharded([[1, 2]], [[OFFSET, OFFSET + 1]])).all()
        idx.add_sparse([[], []])                          # documents, none with tokens: the global N stays 0
        d, r = idx.search_sparse_sharded([1], [1.0], [0, 1], 3)
        assert np.isnan(d).all() and (r == -1).all()
    finally:
        idx.close()


def test_stats_move_as_documented(looped, queries):
    idx, calls = looped
    tq = queries[0][:7]
    distinct = sorted({t for q in tq for t in q if 0 <= t < (1 << 20)})
    idx.search_bm25(tq, 10)
    idx.reset_stats()
    del calls[:]
    idx.search_bm25_sharded(tq, 10)
    assert calls == [8 * (2 + len(distinct)), 8 * 2 * 7 * 10]
    assert idx.stat("sharded_sparse_searches") == 1 and idx.stat("sparse_searches") == 0 and idx.stat("sparse_queries") == 7
    assert idx.stat("shard_gather_bytes") == sum(calls) and idx.stat("sparse_postings_scored") > 0
    idx.search_sparse_subset_sharded([1, 2], [1.0, 0.5], [0, 2], 4, [OFFSET + 1, OFFSET + 2])
    assert calls[2:] == [8 * 2, 8 * 2 * 1 * 4]            # T = 0 for the weighted forms
    assert idx.stat("sharded_sparse_searches") == 2 and idx.stat("sparse_subset_searches") == 0
    del calls[:]
    idx.score_bm25_subset_sharded(tq, np.full((7, 5), OFFSET + 9))
    assert calls == [8 * (2 + len(distinct)), 8 * 7 * 5]
    assert idx.stat("sharded_sparse_scores") == 1 and idx.stat("sparse_subset_scores") == 0
    assert idx.stat("sparse_subset_pairs") >= 35
    # B = 0 is a no-op without a collective
    del calls[:]
    d, r = idx.search_bm25_sharded([], 3)
    assert d.shape == (0, 3) and calls == []


def _refused(fn, code, text):
    from autorag_research_amd._native import NativeError

    with pytest.raises(NativeError, match=text) as e:
        fn()
    assert e.value.code == code


def _entry_calls(idx, buf):
    """one valid call of each of the six entry points (device outputs in `buf`)"""
    ids = [OFFSET + 1, OFFSET + 2]
    return {
        "search_sparse_sharded_device": lambda: idx.search_sparse_sharded_device([1, 2], [1.0, 0.5], [0, 2], 4, buf, buf + 4096),
        "search_bm25_sharded_device": lambda: idx.search_bm25_sharded_device([[1, 2]], 4, buf, buf + 4096),
        "search_sparse_subset_sharded_device": lambda: idx.search_sparse_subset_sharded_device([1, 2], [1.0, 0.5], [0, 2], 4, ids, buf, buf + 4096),
        "search_bm25_subset_sharded_device": lambda: idx.search_bm25_subset_sharded_device([[1, 2]], 4, ids, buf, buf + 4096),
        "score_sparse_subset_sharded": lambda: idx.score_sparse_subset_sharded([1, 2], [1.0, 0.5], [0, 2], [ids]),
        "score_bm25_subset_sharded": lambda: idx.score_bm25_subset_sharded([[1, 2]], [ids]),
    }


def test_refusals_come_before_the_first_collective(looped):
    import autorag_research_amd as pkg

    idx, calls = looped
    sentinel = np.full(1024, 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    buf = idx.dev_alloc(sentinel.nbytes)
    idx.dev_upload(buf, sentinel)
    idx.search_bm25(_token_queries()[:3], 5)
    idx.reset_stats()
    del calls[:]
    keys = ("sharded_sparse_searches", "sharded_sparse_scores", "shard_gather_bytes", "sparse_queries", "sparse_postings_scored",
            "sparse_full_builds", "sparse_overlay_builds")
    try:
        # no communicator
        with pkg.Mi355Index(8) as bare:
            bare.add_sparse([[1, 2], [2, 3]])
            for call in _entry_calls(bare, buf).values():
                _refused(call, E_INVALID, "mi355dr_comm_init has not been called")
            assert all(bare.stat(key) == 0 for key in keys)
        # a view: ask the parent
        with pkg.Mi355Index(8) as parent:
            parent.add(np.random.default_rng(46).standard_normal((64, 8)).astype(np.float32))
            view = parent.view(row_ids=np.arange(10))
            try:
                for call in _entry_calls(view, buf).values():
                    _refused(call, E_INVALID, "ask the parent")
            finally:
                view.close()
        # world * k > 4096, with the world the transport reports: 5 ranks x k = 820
        with pkg.Mi355Index(8) as wide:
            wide.add_sparse([[1, 2], [2, 3]])
            seen = []
            wide.comm_init_custom(2, 5, lambda *a: seen.append(a))
            assert wide.comm_world() == 5
            _refused(lambda: wide.search_bm25_sharded_device([[1, 2]], 820, buf, buf), E_UNSUPPORTED, "exceeds 4096")
            _refused(lambda: wide.search_sparse_subset_sharded_device([1], [1.0], [0, 1], 1024, [0], buf, buf), E_UNSUPPORTED, "exceeds 4096")
            assert seen == [] and all(wide.stat(key) == 0 for key in keys)
        # the local argument errors
        ok_q = ([1, 2], [1.0, 0.5], [0, 2])
        _refused(lambda: idx.search_bm25_sharded_device([[1]], 0, buf, buf), E_INVALID, "k > 0")
        _refused(lambda: idx.search_bm25_sharded_device([[1]], 1025, buf, buf), E_UNSUPPORTED, "exceeds 1024")
        _refused(lambda: idx.search_bm25_sharded_device([[1]], 4, buf, buf, k1=-1.0), E_INVALID, "k1")
        _refused(lambda: idx.search_sparse_sharded_device(*ok_q, 4, buf, buf, b=1.5), E_INVALID, r"b must be in \[0, 1\]")
        _refused(lambda: idx.search_sparse_sharded_device([1, 1], [1.0, 0.5], [0, 2], 4, buf, buf), E_INVALID, "repeated")
        _refused(lambda: idx.search_sparse_sharded_device([1, 1 << 20], [1.0, 0.5], [0, 2], 4, buf, buf), E_INVALID, "term id")
        _refused(lambda: idx.search_sparse_subset_sharded_device([1, 2], [1.0, float("nan")], [0, 2], 4, [0], buf, buf), E_INVALID, "finite")
        _refused(lambda: idx.score_sparse_subset_sharded([1, 1], [1.0, 0.5], [0, 2], [[OFFSET]]), E_INVALID, "repeated")
        _refused(lambda: idx.search_bm25_sharded_device([list(range(1025))], 4, buf, buf), E_UNSUPPORTED, "1024 distinct")
        _refused(lambda: idx.score_bm25_subset_sharded([list(range(1025))], [[OFFSET]]), E_UNSUPPORTED, "1024 distinct")
        _refused(lambda: idx.search_bm25_sharded_device([[1]], 4, 0, buf), E_INVALID, "null buffer")
        lib, h, vp = idx._lib, idx._h, ctypes.c_void_p
        t, off = np.array([1], dtype=np.int32), np.array([0, 1], dtype=np.int32)
        i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))  # noqa: E731
        rc = lib.mi355dr_search_bm25_subset_sharded_device(h, i32(t), i32(off), 1, 4, 1.2, 0.75, None, -1, vp(buf), vp(buf), None)
        assert rc == E_INVALID and b"m must be >= 0" in lib.mi355dr_last_error(h)
        rc = lib.mi355dr_score_bm25_subset_sharded(h, i32(t), i32(off), 1, 1.2, 0.75, None, -1, None)
        assert rc == E_INVALID and b"m must be >= 0" in lib.mi355dr_last_error(h)
        # after every refusal: the transport was never called, no stat moved, no result was written
        assert calls == [] and all(idx.stat(key) == 0 for key in keys)
        back = np.empty_like(sentinel)
        idx.dev_download(buf, back)
        assert np.array_equal(back, sentinel)
    finally:
        idx.dev_free(buf)
