"""GPU: `mi355dr_search_collapsed` / `_device` -- the best k, at most cap per source, deepening only the queries that need it.
The reference is the walk of tests/collapse_ref.py over `idx.search(Q, max_fetch)`, the existing exact search; the corpora are
collapse_ref's (one heavy source in front of one query; a source deeper than max_fetch; a ranking that ends early)."""

import numpy as np
import pytest

import collapse_ref as cr

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -4
K = 10


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


class Case:
    """One corpus in one index under one metric, with the exact search at 1024 taken ONCE."""

    def __init__(self, pkg, corpus, metric):
        self.C, self.Q, self.keys = corpus
        self.idx = pkg.Mi355Index(self.C.shape[1], metric)
        self.idx.add(self.C)
        self.full = self.idx.search(self.Q, 1024)

    def expected(self, cap, k, max_fetch, keys="own"):
        return cr.search_result(self.full[0], self.full[1], self.keys if isinstance(keys, str) else keys, cap, k, max_fetch)

    def close(self):
        self.idx.close()


@pytest.fixture(scope="module", params=["cosine", "ip"])
def case_a(pkg, request):
    c = Case(pkg, cr.corpus_a(), request.param)
    yield c
    c.close()


def test_corpus_a_is_what_the_schedule_tests_need(case_a):
    """Not vacuous: query 0 finds its 10th kept entry some 300 deep, the others within 16 -- on the library's own ranking."""
    for cap, lo in ((1, 307), (2, 306), (3, 305)):
        depth = cr.depth_of_kth(case_a.full[1], case_a.keys, cap, K)
        assert lo <= depth[0] <= lo + 5 and (depth[1:] >= 10).all() and (depth[1:] <= 11).all(), (cap, depth)


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_result_does_not_depend_on_fetch_k(case_a, cap):
    idx = case_a.idx
    exp = case_a.expected(cap, K, 1024)
    assert (exp[3] == K).all() and (exp[4] == 0).all()
    with idx.upload_keys(case_a.keys) as table:
        for fetch_k in (10, 16, 300, 1024):
            want = cr.expected_researched(case_a.full[1], case_a.keys, cap, K, fetch_k, 1024)
            for form, keys in (("host", case_a.keys), ("device", table)):
                idx.reset_stats()
                cr.same_search(idx.search_collapsed(case_a.Q, K, cap, keys, fetch_k, 1024), exp, f"{form} fetch_k={fetch_k}")
                assert idx.stat("collapse_researched") == want, (form, fetch_k)
                assert idx.stat("collapse_searches") == 1 and idx.stat("collapse_queries") == 5
                assert idx.stat("collapse_truncated") == 0


def test_only_the_query_with_the_heavy_source_is_searched_again(case_a):
    idx = case_a.idx
    idx.reset_stats()
    idx.search_collapsed(case_a.Q, K, 1, case_a.keys, 16, 1024)
    assert idx.stat("collapse_researched") == 5            # one query, at 32, 64, 128, 256 and 512
    idx.reset_stats()
    idx.search_collapsed(case_a.Q, K, 1, case_a.keys, 1024, 1024)
    assert idx.stat("collapse_researched") == 0


def test_no_table_is_the_plain_search_bit_for_bit(case_a):
    idx = case_a.idx
    d, r = idx.search(case_a.Q, K)
    for fetch_k in (10, 16):
        got = idx.search_collapsed(case_a.Q, K, 1, None, fetch_k, 1024)
        assert np.array_equal(got.dist.view(np.uint64), d.view(np.uint64)) and np.array_equal(got.rows, r)
        assert (got.keys == -1).all() and (got.count == K).all() and (got.state == 0).all()
    with idx.upload_keys(np.zeros(0, np.int64)) as none:
        got = idx.search_collapsed(case_a.Q, K, 1, none, 16, 1024)
        assert np.array_equal(got.dist.view(np.uint64), d.view(np.uint64)) and np.array_equal(got.rows, r)


def test_max_fetch_that_is_no_power_of_two(case_a):
    idx = case_a.idx
    exp = case_a.expected(1, K, 300)
    assert exp[3][0] < K and exp[4][0] == cr.TRUNCATED and (exp[4][1:] == 0).all()   # query 0: cut inside the heavy source
    for fetch_k in (10, 16, 300):
        idx.reset_stats()
        cr.same_search(idx.search_collapsed(case_a.Q, K, 1, case_a.keys, fetch_k, 300), exp, f"max_fetch=300 fetch_k={fetch_k}")
        assert idx.stat("collapse_truncated") == 1
        assert idx.stat("collapse_researched") == cr.expected_researched(case_a.full[1], case_a.keys, 1, K, fetch_k, 300)
    exp3 = case_a.expected(3, K, 310)
    cr.same_search(idx.search_collapsed(case_a.Q, K, 3, case_a.keys, 16, 310), exp3, "max_fetch=310 cap=3")


def test_1030_queries_cross_a_block_boundary(case_a):
    idx = case_a.idx
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((1030, 64)).astype(np.float32)
    Q[[0, 500, 1023, 1024, 1029]] = case_a.Q[0]            # the heavy source in front of queries of BOTH blocks
    full = idx.search(Q, 512)
    exp = cr.search_result(full[0], full[1], case_a.keys, 1, K, 512)
    want = cr.expected_researched(full[1], case_a.keys, 1, K, 16, 512)
    assert want >= 25
    with idx.upload_keys(case_a.keys) as table:
        for form, keys in (("host", case_a.keys), ("device", table)):
            idx.reset_stats()
            cr.same_search(idx.search_collapsed(Q, K, 1, keys, 16, 512), exp, form + " B=1030")
            assert idx.stat("collapse_researched") == want and idx.stat("collapse_queries") == 1030


def test_a_source_deeper_than_max_fetch_is_truncated(pkg):
    c = Case(pkg, cr.corpus_b(), "cosine")
    try:
        exp = c.expected(1, 2, 1024)
        assert exp[3].tolist() == [2, 1, 2, 2, 2] and exp[4].tolist() == [0, cr.TRUNCATED, 0, 0, 0]
        with c.idx.upload_keys(c.keys) as table:
            for form, keys in (("host", c.keys), ("device", table)):
                c.idx.reset_stats()
                got = c.idx.search_collapsed(c.Q, 2, 1, keys, 2, 1024)
                cr.same_search(got, exp, form)
                assert got.count[1] == 1 and got.state[1] == pkg.index.COLLAPSE_TRUNCATED and got.rows[1, 1] == -1
                assert c.idx.stat("collapse_truncated") == 1
        for k, cap in ((10, 2), (3, 3)):
            cr.same_search(c.idx.search_collapsed(c.Q, k, cap, c.keys, 16, 1024), c.expected(cap, k, 1024), f"k={k} cap={cap}")
    finally:
        c.close()


@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_a_ranking_that_ends_is_finished_at_once(pkg, metric):
    c = Case(pkg, cr.corpus_c(), metric)
    try:
        if metric == "cosine":
            assert np.isnan(c.full[0][:, 47:50]).all() and (c.full[1][:, 47:50] >= 0).all() and (c.full[1][:, 50:] == -1).all()
        for cap in (1, 2, 3):
            exp = c.expected(cap, K, 64)
            assert (exp[4] == 0).all()
            c.idx.reset_stats()
            cr.same_search(c.idx.search_collapsed(c.Q, K, cap, c.keys, 64, 64), exp, f"cap={cap}")
            assert c.idx.stat("collapse_researched") == 0
            cr.same_search(c.idx.search_collapsed(c.Q, K, cap, c.keys, 10, 1024), c.expected(cap, K, 1024), f"cap={cap} from 10")
        # more asked for than one source each can give: 13 sources, the NaN rows among the kept entries, not truncated
        exp = c.expected(1, 20, 64)
        assert (exp[3] == 13).all() and (exp[4] == 0).all()
        cr.same_search(c.idx.search_collapsed(c.Q, 20, 1, c.keys, 20, 64), exp, "k above the sources")
    finally:
        c.close()


def test_after_remove_rows_and_after_compact(pkg):
    C, Q, keys = cr.corpus_a()
    with pkg.Mi355Index(64) as idx:
        idx.add(C)
        gone = np.r_[np.arange(1000, 1300, 2), 5, 4000].astype(np.int64)   # half of the planted rows and two others
        idx.remove_rows(gone)
        full = idx.search(Q, 1024)
        assert not np.isin(full[1], gone).any()
        exp = cr.search_result(full[0], full[1], keys, 1, K, 1024)
        for fetch_k in (16, 1024):
            cr.same_search(idx.search_collapsed(Q, K, 1, keys, fetch_k, 1024), exp, f"removed fetch_k={fetch_k}")
        new_of_old = idx.compact()
        rekeyed = np.full(len(idx), -1, dtype=np.int64)
        rekeyed[new_of_old[new_of_old >= 0]] = keys[new_of_old >= 0]
        full = idx.search(Q, 1024)
        exp2 = cr.search_result(full[0], full[1], rekeyed, 1, K, 1024)
        assert np.array_equal(exp2[2], exp[2])   # (the same sources in the same order: only the ids were renumbered)
        for fetch_k in (16, 1024):
            cr.same_search(idx.search_collapsed(Q, K, 1, rekeyed, fetch_k, 1024), exp2, f"compacted fetch_k={fetch_k}")


def test_on_a_view_keyed_with_the_parents_ids(case_a):
    listed = np.r_[np.arange(0, 4096, 2), np.arange(1001, 1300, 2)].astype(np.int64)   # every even row and the odd planted rows
    with case_a.idx.view(row_ids=listed) as v:
        full = v.search(case_a.Q, 1024)
        assert np.isin(full[1][full[1] >= 0], listed).all() and (full[1] >= 0).all()
        for cap in (1, 2):
            exp = cr.search_result(full[0], full[1], case_a.keys, cap, K, 1024)
            for fetch_k in (16, 1024):
                v.reset_stats()
                cr.same_search(v.search_collapsed(case_a.Q, K, cap, case_a.keys, fetch_k, 1024), exp, f"view cap={cap} f={fetch_k}")
                assert v.stat("collapse_researched") == cr.expected_researched(full[1], case_a.keys, cap, K, fetch_k, 1024)


def test_default_fetch_k_and_the_search_in_flight(pkg, case_a):
    idx = case_a.idx
    exp = case_a.expected(1, K, 1024)
    cr.same_search(idx.search_collapsed(case_a.Q, K, 1, case_a.keys), exp, "default fetch_k")
    assert pkg.Mi355Index.collapse_fetch_k(10, None, 1024) == pkg.index.COLLAPSE_FETCH_MULT * 10
    assert pkg.Mi355Index.collapse_fetch_k(10, None, 12) == min(12, pkg.index.COLLAPSE_FETCH_MULT * 10)   # within [k, max_fetch]
    assert pkg.Mi355Index.collapse_fetch_k(10, 64, 1024) == 64
    # a block still in flight is completed first, and its results are the plain search's
    Q = case_a.Q
    bufs = [idx.dev_alloc(Q.nbytes), idx.dev_alloc(5 * K * 8), idx.dev_alloc(5 * K * 8)]
    try:
        idx.dev_upload(bufs[0], Q)
        ticket = idx.search_device_async(bufs[0], 5, K, bufs[1], bufs[2])
        cr.same_search(idx.search_collapsed(Q, K, 1, case_a.keys, 16, 1024), exp, "behind a block in flight")
        idx.search_wait(ticket)
        d, r = np.empty((5, K)), np.empty((5, K), np.int64)
        idx.dev_download(bufs[1], d)
        idx.dev_download(bufs[2], r)
        pd, pr = idx.search(Q, K)
        assert np.array_equal(d.view(np.uint64), pd.view(np.uint64)) and np.array_equal(r, pr)
    finally:
        for b in bufs:
            idx.dev_free(b)


def test_refusals_change_nothing(pkg, case_a):
    idx, Q, keys = case_a.idx, case_a.Q, case_a.keys
    idx.reset_stats()
    bad = [
        (dict(k=0), E_INVALID), (dict(cap=0), E_INVALID), (dict(fetch_k=9), E_INVALID), (dict(fetch_k=64, max_fetch=32), E_INVALID),
        (dict(max_fetch=1025), E_UNSUPPORTED), (dict(k=1025, fetch_k=1025, max_fetch=1025), E_UNSUPPORTED),
    ]
    for change, code in bad:
        a = dict(k=K, cap=1, fetch_k=16, max_fetch=1024)
        a.update(change)
        with pytest.raises(pkg.NativeError) as e:
            idx.search_collapsed(Q, a["k"], a["cap"], keys, a["fetch_k"], a["max_fetch"])
        assert e.value.code == code, change
    assert idx.stat("collapse_searches") == 0 and idx.stat("passes") == 0
    got = idx.search_collapsed(np.zeros((0, 64), np.float32), K, 1, keys, 16, 1024)   # B == 0: a no-op
    assert got.rows.shape == (0, K) and idx.stat("collapse_searches") == 0
    with pytest.raises(pkg.NativeError) as e:                                         # no communicator on this index
        idx.search_collapsed_sharded(Q, K, 1, keys, 16, 1024)
    assert e.value.code == E_INVALID
