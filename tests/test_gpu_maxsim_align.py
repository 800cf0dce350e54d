"""GPU parity: "MaxSim explained" -- mi355dr_maxsim_align / _maxsim_map / _multivec_token_counts against the reference
(tests/maxsim_align_ref.py).  Every value is compared as uint32 bits, every token index exactly, and `dist` with
`maxsim_subset` of the same call.  All stores are under 300 documents."""

import ctypes

import numpy as np
import pytest

import maxsim_align_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
E_INVALID, E_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def _unit(rng, n, d):
    v = rng.standard_normal((n, d)).astype(F32)
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-30).astype(F32)


def _flat(docs, d):
    tok = np.concatenate(docs, axis=0) if docs else np.zeros((0, d), F32)
    return tok.reshape(-1, d), np.concatenate([[0], np.cumsum([t.shape[0] for t in docs])]).astype(np.int64)


def _qoff(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


class Pair:
    """the index under test and the reference store with the same contents: every change goes to both"""

    def __init__(self, pkg, docs, d, row_offset=0):
        self.d, self.idx, self.ref = d, pkg.Mi355Index(d), ref.RefStore(d)
        if row_offset:
            self.idx.set_option("row_offset", row_offset)
            self.ref.set_option("row_offset", row_offset)
        self.add(docs)

    def add(self, docs):
        for s in (self.idx, self.ref):
            s.add_multivec(*_flat(docs, self.d))

    def set(self, ids, docs):
        for s in (self.idx, self.ref):
            s.set_multivec(np.asarray(ids, dtype=np.int64), *_flat(docs, self.d))

    def check(self, q, qoff, ids, clamp0=False):
        """align == reference, dist == maxsim_subset of the same call, want_dist=False gives the same values"""
        ids = np.asarray(ids, dtype=np.int64)
        got = self.idx.maxsim_align(q, qoff, ids, clamp0=clamp0)
        ref.same_alignment(got, self.ref.maxsim_align(q, qoff, ids, clamp0=clamp0))
        ref.same_bits(got.dist, self.idx.maxsim_subset(q, qoff, ids, clamp0=clamp0))
        for b in range(ids.shape[0]):     # -value summed in a Python fp32 loop in vector order: the same bits again
            for p in range(ids.shape[1]):
                if not np.isnan(got.dist[b, p]):
                    assert ref.fold(got.values[qoff[b]:qoff[b + 1], p]).view(np.uint32) == got.dist[b, p].view(np.uint32)
        bare = self.idx.maxsim_align(q, qoff, ids, clamp0=clamp0, want_dist=False)
        assert bare.dist is None
        ref.same_bits(bare.values, got.values)
        assert np.array_equal(bare.tokens, got.tokens)
        return got

    def close(self):
        self.idx.close()


# documents of the main store (d = 128), by position
LENS = [1, 31, 32, 33, 64, 65, 150, 0, 33, 65, 50, 150, 32]
P_EMPTY, P_LAST33, P_LAST65, P_DUP50, P_DUP150, P_ROWS = 7, 8, 9, 10, 11, 12


@pytest.fixture(scope="module")
def main(pkg):
    rng = np.random.default_rng(2024)
    docs = [_unit(rng, t, 128) for t in LENS]
    docs[P_DUP50][9] = docs[P_DUP50][5]          # a tie inside one block
    docs[P_DUP50][40] = docs[P_DUP50][3]         # ... across adjacent blocks
    docs[P_DUP150][42] = docs[P_DUP150][10]      # ... across blocks 0, 1 and 4
    docs[P_DUP150][138] = docs[P_DUP150][10]
    p = Pair(pkg, docs, 128)
    yield p, docs
    p.close()


@pytest.mark.parametrize("clamp0", [False, True])
def test_lengths_queries_and_id_hygiene(main, clamp0):
    """every document length against queries of 1, 32, 33, 0 and 7 vectors (B = 5, m = 7); ids out of range, negative, -1
    padding, an empty document and the same document twice in a row"""
    p, docs = main
    rng = np.random.default_rng(1)
    qlens = [1, 32, 33, 0, 7]
    q = _unit(rng, sum(qlens), 128)
    ids = np.array([[0, 1, 2, 3, 4, 5, 6],
                    [6, P_EMPTY, 3, 3, -1, len(LENS), 2],
                    [5, -9, 0, 1, 2**40, 4, 5],
                    [0, 1, 2, 3, 4, 5, 6],
                    [12, 11, 10, 9, 8, -1, -1]], dtype=np.int64)
    got = p.check(q, _qoff(qlens), ids, clamp0)
    assert got.values.shape == (73, 7) and np.all(np.isnan(got.dist[3]))           # the empty query owns no rows
    assert np.all(np.isnan(got.values[1:33, 1])) and np.all(got.tokens[1:33, 1] == -1)   # the empty document
    assert np.array_equal(got.tokens[1:33, 2], got.tokens[1:33, 3])                # scored per position
    for b, row in enumerate(ids):   # never a padded copy
        for pos, i in enumerate(row):
            if 0 <= i < len(LENS):
                assert got.tokens[_qoff(qlens)[b]:_qoff(qlens)[b + 1], pos].max(initial=-1) < max(LENS[i], 1)


def test_one_query_one_candidate_and_129_vectors(main):
    """B = 1, m = 1; a query of 129 vectors at d = 128 is scored in two tiles (128 + 1)"""
    p, docs = main
    rng = np.random.default_rng(2)
    p.check(_unit(rng, 1, 128), _qoff([1]), [[5]])
    got = p.check(_unit(rng, 129, 128), _qoff([129]), [[3, 6, 0]])
    assert got.values.shape == (129, 3)


def test_every_accumulator_row_wins_once(main):
    """a document of 32 tokens, query vector j = token j: token j must win, for every row of the MFMA's C/D layout"""
    p, docs = main
    got = p.check(docs[P_ROWS].copy(), _qoff([32]), [[P_ROWS]])
    assert np.array_equal(got.tokens[:, 0], np.arange(32))
    # ... and in the second and fifth block of a longer document
    sel = np.r_[32:64, 128:150]
    got = p.check(docs[6][sel].copy(), _qoff([sel.size]), [[6]])
    assert np.array_equal(got.tokens[:, 0], sel)


def test_exact_ties_take_the_lowest_index(main):
    p, docs = main
    q = np.stack([docs[P_DUP50][5], docs[P_DUP50][3], docs[P_DUP50][9], docs[P_DUP50][40]])
    got = p.check(q, _qoff([4]), [[P_DUP50]])
    assert got.tokens[:, 0].tolist() == [5, 3, 5, 3]
    q = np.stack([docs[P_DUP150][10], docs[P_DUP150][138], docs[P_DUP150][42]])
    got = p.check(q, _qoff([3]), [[P_DUP150, P_DUP50]])
    assert got.tokens[:, 0].tolist() == [10, 10, 10]


def test_best_token_is_the_last_one(main):
    """T = 33 and T = 65: the padded copies of the last token tie with it and must lose"""
    p, docs = main
    q = np.stack([docs[P_LAST33][32], docs[P_LAST65][64]])
    got = p.check(q, _qoff([2]), [[P_LAST33, P_LAST65]])
    assert got.tokens[0, 0] == 32 and got.tokens[1, 1] == 64


def test_non_finite_tokens_and_clamp_of_negative_dots(pkg):
    rng = np.random.default_rng(3)
    d = 128
    u = _unit(rng, 3, d)
    nan_tok = _unit(rng, 40, d)
    nan_tok[4] = np.nan
    nan_tok[35] = np.nan
    neg = -(u[0] + 0.05 * _unit(rng, 37, d))          # every dot with u[0] is negative
    p = Pair(pkg, [nan_tok, np.full((3, d), np.nan, F32), neg], d)
    try:
        got = p.check(u, _qoff([3]), [[0, 1, 2]])
        assert not np.any(np.isin(got.tokens[:, 0], [4, 35])) and np.all(got.tokens[:, 0] >= 0)   # a NaN token is ignored
        assert np.all(np.isneginf(got.values[:, 1])) and np.all(got.tokens[:, 1] == -1)            # nothing but NaN
        got_c = p.check(u[:1], _qoff([1]), [[2, 1]], clamp0=True)
        assert got.values[0, 2] < 0 and got_c.values[0, 0] == 0.0 and got_c.tokens[0, 0] == got.tokens[0, 2]
    finally:
        p.close()


@pytest.mark.parametrize("d,qlens", [(20, [5, 33]), (768, [40, 3])])
def test_other_dims(pkg, d, qlens):
    """d = 20 is padded to 24 (zero columns); d = 768 stages 32 columns per launch: a 40-vector query is tiled (32 + 8)"""
    rng = np.random.default_rng(d)
    docs = [_unit(rng, t, d) for t in (33, 65, 5, 0, 32)]
    p = Pair(pkg, docs, d)
    try:
        q = _unit(rng, sum(qlens), d)
        q[0] = docs[1][64]
        got = p.check(q, _qoff(qlens), [[0, 1, 2, 3], [4, 1, -1, 0]])
        assert got.tokens[0, 1] == 64
        maps = p.idx.maxsim_map(q, _qoff(qlens), [0, 1], [1, 4])
        for a, b in zip(maps, p.ref.maxsim_map(q, _qoff(qlens), [0, 1], [1, 4])):
            ref.same_bits(a, b)
    finally:
        p.close()


def test_row_offset_and_mutation(pkg):
    """global ids under "row_offset"; a document removed by set_multivec, revived with another length (the relayout path), then
    rewritten in place: token indices refer to the new contents"""
    rng = np.random.default_rng(4)
    d, off = 128, 1000
    docs = [_unit(rng, t, d) for t in (40, 33, 70, 5)]
    p = Pair(pkg, docs, d, row_offset=off)
    try:
        q = _unit(rng, 6, d)
        qo = _qoff([4, 2])
        ids = np.array([[off, off + 1, off + 2, off + 3, 1, off + 4, -1], [off + 2] * 7], dtype=np.int64)
        p.check(q, qo, ids)
        assert np.array_equal(p.idx.multivec_token_counts([off, off + 3, off + 4, 0, -1]), [40, 5, -1, -1, -1])
        p.set([1], [np.zeros((0, d), F32)])                       # removed
        got = p.check(q, qo, ids)
        assert np.all(np.isnan(got.values[:4, 1])) and p.idx.multivec_token_counts([off + 1])[0] == 0
        new = _unit(rng, 90, d)                                   # revived, three blocks instead of two
        q[0] = new[77]
        p.set([1], [new])
        assert p.idx.stat("maxsim_moved_blocks") > 0
        got = p.check(q, qo, ids)
        assert got.tokens[0, 1] == 77
        moved = p.idx.stat("maxsim_moved_blocks")
        again = _unit(rng, 70, d)                                 # in place: still three blocks
        q[1] = again[69]
        p.set([1], [again])
        assert p.idx.stat("maxsim_moved_blocks") == moved
        got = p.check(q, qo, ids)
        assert got.tokens[1, 1] == 69
        ref.same_bits(p.idx.maxsim_map(q, qo, [0], [off + 1])[0], ref.dots(q[:4], again))
    finally:
        p.close()


def _raw_map(idx, q, qo, pq, pd, off, out):
    q, qo = np.ascontiguousarray(q, F32), np.ascontiguousarray(qo, np.int32)
    pq, pd, off = np.ascontiguousarray(pq, np.int32), np.ascontiguousarray(pd, np.int64), np.ascontiguousarray(off, np.int64)
    P = ctypes.POINTER
    return idx._lib.mi355dr_maxsim_map(idx._h, q.ctypes.data_as(P(ctypes.c_float)), qo.ctypes.data_as(P(ctypes.c_int32)), qo.size - 1,
                                       pq.ctypes.data_as(P(ctypes.c_int32)), pd.ctypes.data_as(P(ctypes.c_int64)), pq.size,
                                       off.ctypes.data_as(P(ctypes.c_int64)), out.ctypes.data_as(P(ctypes.c_float)))


def test_maps(main):
    """every element against the oracle's dot; row maxima and first argmax against maxsim_align of the same pair; two pairs
    sharing a query, an empty slot for an empty document, a wrong slot size refused with nothing written; token counts"""
    p, docs = main
    rng = np.random.default_rng(6)
    qlens = [7, 0, 33]
    q, qo = _unit(rng, 40, 128), _qoff(qlens)
    pq, pd = [0, 0, 2, 2, 1, 0, 2], [6, 3, 6, P_EMPTY, 3, 99, P_DUP50]
    before = p.idx.stat("maxsim_map_values")
    maps = p.idx.maxsim_map(q, qo, pq, pd)
    want = p.ref.maxsim_map(q, qo, pq, pd)
    assert [m.shape for m in maps] == [(7, 150), (7, 33), (33, 150), (33, 0), (0, 33), (7, 0), (33, 50)]
    for a, b in zip(maps, want):
        ref.same_bits(a, b)
    assert p.idx.stat("maxsim_map_values") - before == sum(m.size for m in maps)
    al = p.idx.maxsim_align(q, qo, [[6, 3], [0, 0], [6, P_DUP50]])
    for m, rows, pos in ((maps[0], slice(0, 7), 0), (maps[1], slice(0, 7), 1), (maps[2], slice(7, 40), 0), (maps[6], slice(7, 40), 1)):
        ref.same_bits(m.max(axis=1), al.values[rows, pos])
        assert np.array_equal(m.argmax(axis=1), al.tokens[rows, pos])
    assert np.array_equal(p.idx.multivec_token_counts([6, P_EMPTY, len(LENS), -1, 0]), [150, 0, -1, -1, 1])
    # a slot of the wrong size: refused, nothing written
    out = np.full(7 * 150 + 8, 123.0, dtype=F32)
    for off in ([0, 7 * 150 - 1], [0, 7 * 150 + 1], [0, 0]):
        assert _raw_map(p.idx, q, qo, [0], [6], off, out) == E_INVALID
    assert _raw_map(p.idx, q, qo, [1], [6], [0, 150], out) == E_INVALID        # a query without vectors, a non-empty slot
    assert _raw_map(p.idx, q, qo, [3], [6], [0, 0], out) == E_INVALID          # pair_query out of range
    assert _raw_map(p.idx, q, qo, [-1], [6], [0, 0], out) == E_INVALID
    assert np.all(out == 123.0)
    assert _raw_map(p.idx, q, qo, [0], [6], [4, 4 + 7 * 150], out) == 0        # offsets need not start at 0
    ref.same_bits(out[4:4 + 7 * 150].reshape(7, 150), want[0])
    assert np.all(out[:4] == 123.0) and np.all(out[4 + 7 * 150:] == 123.0)


def test_errors_refusals_and_no_ops(main, pkg):
    p, docs = main
    idx = p.idx
    L, h, P = idx._lib, idx._h, ctypes.POINTER
    q = np.ascontiguousarray(docs[2][:4])
    qo = np.array([0, 1, 4], dtype=np.int32)
    ids = np.array([[0, 1], [2, 3]], dtype=np.int64)
    val, tok, dist = np.full((4, 2), 5.0, F32), np.full((4, 2), 5, np.int32), np.full((2, 2), 5.0, F32)
    fp, ip, lp = (lambda a: a.ctypes.data_as(P(ctypes.c_float))), (lambda a: a.ctypes.data_as(P(ctypes.c_int32))), \
        (lambda a: a.ctypes.data_as(P(ctypes.c_int64)))
    bad_qo = np.array([0, 3, 2], dtype=np.int32)
    calls = {
        "unknown flag": lambda: L.mi355dr_maxsim_align(h, fp(q), ip(qo), 2, lp(ids), 2, 2, fp(val), ip(tok), fp(dist)),
        "B < 0": lambda: L.mi355dr_maxsim_align(h, fp(q), ip(qo), -1, lp(ids), 2, 0, fp(val), ip(tok), fp(dist)),
        "m < 0": lambda: L.mi355dr_maxsim_align(h, fp(q), ip(qo), 2, lp(ids), -1, 0, fp(val), ip(tok), fp(dist)),
        "null ids": lambda: L.mi355dr_maxsim_align(h, fp(q), ip(qo), 2, None, 2, 0, fp(val), ip(tok), fp(dist)),
        "null values": lambda: L.mi355dr_maxsim_align(h, fp(q), ip(qo), 2, lp(ids), 2, 0, None, ip(tok), fp(dist)),
        "null tokens": lambda: L.mi355dr_maxsim_align(h, fp(q), ip(qo), 2, lp(ids), 2, 0, fp(val), None, fp(dist)),
        "null queries": lambda: L.mi355dr_maxsim_align(h, None, ip(qo), 2, lp(ids), 2, 0, fp(val), ip(tok), fp(dist)),
        "null offsets": lambda: L.mi355dr_maxsim_align(h, fp(q), None, 2, lp(ids), 2, 0, fp(val), ip(tok), fp(dist)),
        "decreasing offsets": lambda: L.mi355dr_maxsim_align(h, fp(q), ip(bad_qo), 2, lp(ids), 2, 0, fp(val), ip(tok), fp(dist)),
        "map: P < 0": lambda: L.mi355dr_maxsim_map(h, fp(q), ip(qo), 2, ip(tok), lp(ids), -1, lp(ids), fp(val)),
        "map: null pairs": lambda: L.mi355dr_maxsim_map(h, fp(q), ip(qo), 2, None, lp(ids), 1, lp(ids), fp(val)),
        "map: decreasing offsets": lambda: L.mi355dr_maxsim_map(h, fp(q), ip(bad_qo), 2, ip(tok), lp(ids), 0, lp(ids), fp(val)),
        "counts: n < 0": lambda: L.mi355dr_multivec_token_counts(h, lp(ids), -1, ip(tok)),
        "counts: null": lambda: L.mi355dr_multivec_token_counts(h, None, 2, ip(tok)),
    }
    for name, call in calls.items():
        assert call() == E_INVALID, name
    assert np.all(val == 5.0) and np.all(tok == 5) and np.all(dist == 5.0)
    # no-ops still fill what they own
    assert L.mi355dr_maxsim_align(h, fp(q), ip(qo), 2, lp(ids), 0, 0, fp(val), ip(tok), fp(dist)) == 0
    assert L.mi355dr_maxsim_align(h, fp(q), ip(qo), 0, lp(ids), 2, 0, fp(val), ip(tok), fp(dist)) == 0
    assert L.mi355dr_maxsim_map(h, fp(q), ip(qo), 2, None, None, 0, None, None) == 0
    assert np.all(val == 5.0)
    got = idx.maxsim_align(q, np.array([0, 0, 0], np.int32), ids)      # no vectors at all: NaN distances, no value rows
    assert got.values.shape == (0, 2) and np.all(np.isnan(got.dist))
    assert L.mi355dr_maxsim_align(h, fp(q), ip(qo), 2, lp(ids), 2, 0, fp(val), ip(tok), None) == 0    # dist not wanted
    assert not np.any(np.isnan(val)) and np.all(tok >= 0)
    # an index without a multi-vector store: everything skipped
    with pkg.Mi355Index(128) as bare:
        got = bare.maxsim_align(q, qo, ids)
        assert np.all(np.isnan(got.values)) and np.all(got.tokens == -1) and np.all(np.isnan(got.dist))
        assert bare.multivec_token_counts([0, 1]).tolist() == [-1, -1]
        assert [m.shape for m in bare.maxsim_map(q, qo, [0, 1], [0, 5])] == [(1, 0), (3, 0)]
    # a view refuses and points at the parent
    with idx.view(doc_ids=np.arange(4)) as v:
        for call in (lambda: v.maxsim_align(q, qo, ids), lambda: v.maxsim_map(q, qo, [0], [1]), lambda: v.multivec_token_counts([0])):
            with pytest.raises(pkg.NativeError) as e:
                call()
            assert e.value.code == E_INVALID and "parent" in str(e.value)
    # the dim bound of the exact kernel
    with pkg.Mi355Index(1280) as wide:
        wide.add_multivec(np.ones((2, 1280), F32), [0, 2])
        with pytest.raises(pkg.NativeError) as e:
            wide.maxsim_align(np.ones((1, 1280), F32), [0, 1], [[0]])
        assert e.value.code == E_UNSUPPORTED


def test_neighbours_undisturbed_and_stats(main):
    """search_maxsim, maxsim_subset and search_maxsim_subset give identical bits before and after an align / map call, and
    their stats do not move; the four new stats count calls, scored pairs and floats written"""
    p, docs = main
    idx = p.idx
    rng = np.random.default_rng(8)
    qlens = [32, 5, 0]
    q, qo = _unit(rng, 37, 128), _qoff(qlens)
    ids = np.array([[0, 6, P_EMPTY, -1], [3, 3, 99, 5], [1, 2, 3, 4]], dtype=np.int64)
    sub = np.arange(len(LENS), dtype=np.int64)

    def neighbours():
        return idx.search_maxsim(q, qo, 5), idx.maxsim_subset(q, qo, ids), idx.search_maxsim_subset(q, qo, 5, sub)

    old = [k for k in ("maxsim_screened", "maxsim_candidates", "maxsim_fallbacks", "maxsim_screen_launches", "maxsim_exact_launches",
                       "maxsim_subset_searches", "maxsim_subset_docs", "maxsim_subset_screened", "maxsim_subset_exact",
                       "maxsim_subset_fallbacks", "maxsim_set_docs", "maxsim_moved_blocks")]
    a = neighbours()
    s0 = {k: idx.stat(k) for k in old}
    n0 = {k: idx.stat(k) for k in ("maxsim_align_calls", "maxsim_align_pairs", "maxsim_map_calls", "maxsim_map_values")}
    idx.maxsim_align(q, qo, ids)
    idx.maxsim_map(q, qo, [0, 1], [6, 3])
    assert {k: idx.stat(k) for k in old} == s0
    n1 = {k: idx.stat(k) - n0[k] for k in n0}
    # scored pairs: query 0 -> docs 0, 6; query 1 -> 3, 3, 5; query 2 has no vectors
    assert n1 == {"maxsim_align_calls": 1, "maxsim_align_pairs": 5, "maxsim_map_calls": 1, "maxsim_map_values": 32 * 150 + 5 * 33}
    b = neighbours()
    for (da, ra), (db, rb) in ((a[0], b[0]), (a[2], b[2])):
        assert np.array_equal(ra, rb)
        ref.same_bits(da, db)
    ref.same_bits(a[1], b[1])


class OneRank:
    """torch.distributed's all-gather for a world of one"""

    @staticmethod
    def all_gather_into_tensor(out, mine, group=None):
        out.copy_(mine)


def test_sharded_searcher_world_one_through_the_pipeline(main, pkg):
    from autorag_research_amd.sharded import ShardedSearcher

    p, docs = main
    rng = np.random.default_rng(9)
    q, qo = _unit(rng, 9, 128), _qoff([4, 0, 5])
    ids = np.array([[0, 5, P_EMPTY], [1, 2, 3], [-1, 99, 6]], dtype=np.int64)
    s = ShardedSearcher(128, "cosine", 0)
    try:
        s.add_local_multivec(*_flat(docs, 128), 500)
        s._dist, s.force_pipeline = OneRank, True
        want = p.idx.maxsim_align(q, qo, ids)
        ref.same_alignment(s.maxsim_align(q, qo, ids + 500), want)
        shifted = np.where(ids >= 0, ids + 500, ids)
        assert np.array_equal(s.multivec_token_counts(shifted.reshape(-1)), p.idx.multivec_token_counts(ids.reshape(-1)))
        for a, b in zip(s.maxsim_map(q, qo, [0, 2, 1], [506, 503, 503]), p.idx.maxsim_map(q, qo, [0, 2, 1], [6, 3, 3])):
            ref.same_bits(a, b)
    finally:
        s.close()


def test_service_on_a_real_index(pkg):
    from helpers import build_golden_stores

    from autorag_research_amd.service import Mi355RetrievalService

    store, g = build_golden_stores()
    s = Mi355RetrievalService(lambda: store)
    ids = list(g["ids"])
    with_mv = [pk for pk, m in zip(ids, g["multivec"]) if m is not None and len(m)]
    q = np.asarray(g["Qm"][0], dtype=F32)
    asked = with_mv[:4] + ["no such id"]
    scores = s.maxsim_score_candidates(q, asked)
    ex = s.maxsim_explain(q, asked)
    assert set(ex) == set(scores) == set(with_mv[:4])
    for pk in ex:
        dd = ref.dots(q, np.asarray(g["multivec"][ids.index(pk)], dtype=F32))
        assert ex[pk]["score"] == scores[pk]
        ref.same_bits(ex[pk]["token_scores"], dd.max(axis=1))
        assert np.array_equal(ex[pk]["token_matches"], dd.argmax(axis=1))
        ref.same_bits(s.maxsim_similarity_map(q, pk), dd)
    assert s.maxsim_explain(q, ["no such id"]) == {} and s.maxsim_similarity_map(q, "no such id") is None
