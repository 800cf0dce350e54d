"""CPU: the numpy restatement of the search by stored row (tests/rows_ref.py) against a brute-force double loop, the
declaration and binding of the four entry points, and the service's `similar_chunks` over a stand-in index that answers
`search_rows` / `search_range_rows` from the reference."""

import re
from pathlib import Path

import numpy as np
import pytest

import range_ref
import rows_ref
from helpers import OracleIndex, build_golden_stores

ROOT = Path(__file__).resolve().parent.parent
NAN, INF = float("nan"), float("inf")
NAMES = ("mi355dr_search_rows", "mi355dr_search_rows_device", "mi355dr_search_range_rows", "mi355dr_search_range_rows_device")


# ---- the reference itself, against a double loop ----------------------------------------------------------------------------

def small_corpus():
    rng = np.random.default_rng(40)
    C = rng.standard_normal((40, 12)).astype(np.float32)
    C[3] = 0.0                                   # zero row: NaN to everything under cosine
    C[20] = C[21] = C[33] = C[8]                 # four exact copies
    C[30] = 2.0 * C[11]                          # same direction, another norm
    live = np.ones(40, dtype=bool)
    live[[8, 15, 39]] = False                    # a removed copy, a removed ordinary row, the removed last row
    return C, live


def pair_distance(oracle, C, a, b, metric):
    return oracle.topk_search(C[b:b + 1], C[a:a + 1], 1, metric=metric, threads=1)[0][0, 0]   # (one pair: no thread team)


def brute_lists(oracle, C, live, metric):
    """per row a: every live row b in the total order, as [(distance, b)] -- one oracle call per pair"""
    out = []
    for a in range(len(C)):
        pairs = [(pair_distance(oracle, C, a, b, metric), b) for b in range(len(C)) if live[b]]
        out.append(sorted(pairs, key=lambda p: (np.isnan(p[0]), 0.0 if np.isnan(p[0]) else p[0], p[1])))
    return out


@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_ref_equals_a_double_loop(oracle, metric):
    C, live = small_corpus()
    lists = brute_lists(oracle, C, live, metric)
    ids = np.array([0, 8, 20, 21, 33, 3, 30, 11, 15, 39, -1, 40, 45, -7, 20, 0])
    for include_self in (False, True):
        for k in (1, 2, 3, 10, 50):
            d, r = rows_ref.search_rows(oracle, C, ids, k, metric, live, include_self)
            assert d.shape == r.shape == (len(ids), k)
            for b, a in enumerate(ids.tolist()):
                if not (0 <= a < 40) or not live[a]:
                    assert (r[b] == -1).all() and np.isnan(d[b]).all()
                    continue
                want = [p for p in lists[a] if include_self or p[1] != a][:k]
                assert r[b, :len(want)].tolist() == [p[1] for p in want] and (r[b, len(want):] == -1).all()
                wd = np.array([p[0] for p in want])
                assert np.array_equal(np.isnan(d[b, :len(want)]), np.isnan(wd)) and np.isnan(d[b, len(want):]).all()
                ok = ~np.isnan(wd)
                assert np.array_equal(d[b, :len(want)][ok].view(np.uint64), wd[ok].view(np.uint64))
        # the range form: counts and lists from the same lists
        radius = np.resize(np.array([INF, -INF, 0.0, 0.5, 1e-7, 1.0]), len(ids))
        for m in (1, 3, 50):
            d, r, c = rows_ref.search_range_rows(oracle, C, ids, radius, m, metric, live, include_self)
            for b, a in enumerate(ids.tolist()):
                if not (0 <= a < 40) or not live[a]:
                    assert c[b] == 0 and (r[b] == -1).all() and np.isnan(d[b]).all()
                    continue
                want = [p for p in lists[a] if (include_self or p[1] != a) and p[0] <= radius[b]]
                assert c[b] == len(want) and r[b, :min(m, len(want))].tolist() == [p[1] for p in want[:m]]
                assert (r[b, len(want):] == -1).all()
                assert d[b, :min(m, len(want))].view(np.uint64).tolist() == [np.float64(p[0]).view(np.uint64) for p in want[:m]]


def test_ref_duplicate_corner_and_offsets(oracle):
    """more than k copies at lower ids: the row itself lies behind the top-(k + 1) list, and the answer is that list cut to k"""
    C, _ = small_corpus()
    full = oracle.topk_search(C, C[33:34], 4)[1][0].tolist()
    assert full == [8, 20, 21, 33]
    assert rows_ref.search_rows(oracle, C, [33], 2)[1].tolist() == [[8, 20]]
    assert rows_ref.search_rows(oracle, C, [33], 3)[1].tolist() == [[8, 20, 21]]
    assert rows_ref.search_rows(oracle, C, [8], 1)[1].tolist() == [[20]]
    assert rows_ref.search_rows(oracle, C, [33], 2, include_self=True)[1].tolist() == [[8, 20]]
    # the zero row under cosine: all NaN in row order, itself taken out
    d, r = rows_ref.search_rows(oracle, C, [3], 5)
    assert r.tolist() == [[0, 1, 2, 4, 5]] and np.isnan(d).all()
    # the range form with the duplicates' own distance as the radius, and the next double below it
    dup = oracle.topk_search(C, C[33:34], 1)[0][0, 0]
    assert rows_ref.search_range_rows(oracle, C, [33], dup, 2)[2].tolist() == [3]
    assert rows_ref.search_range_rows(oracle, C, [33], dup, 2, include_self=True)[2].tolist() == [4]
    assert rows_ref.search_range_rows(oracle, C, [33], np.nextafter(dup, -INF), 2)[2].tolist() == [0]
    # global ids: accepted and returned with the offset, ids below it are no rows of the index
    d0, r0 = rows_ref.search_rows(oracle, C, [33, 7], 3)
    d1, r1 = rows_ref.search_rows(oracle, C, [5033, 5007, 33], 3, row_offset=5000)
    assert np.array_equal(r1[:2], r0 + 5000) and (r1[2] == -1).all()
    rows_ref.same((d1[:2], r1[:2] - 5000), (d0, r0))
    with pytest.raises(AssertionError):
        rows_ref.same((d0, r0), (d0, r0[:, ::-1].copy()))


# ---- the ABI and its binding ---------------------------------------------------------------------------------------------------

def test_header_declares_and_native_binds_the_four_entry_points(native_built):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mi355dr.h").read_text(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    assert re.search(r"#define\s+MI355DR_ROWS_INCLUDE_SELF\s+1\b", text)
    from autorag_research_amd import _native

    assert set(NAMES) <= set(_native.ABI_SYMBOLS)
    lib = _native.load()
    assert [len(getattr(lib, name).argtypes) for name in NAMES] == [7, 8, 9, 10]


def test_wrappers_check_shapes_before_the_library():
    from autorag_research_amd.index import Mi355Index

    class Unreached(Mi355Index):   # (no handle: the checks come before the first use of the library)
        def __init__(self):
            self.dim = 4

        def __del__(self):
            pass

        def __len__(self):
            return 10

    ix = Unreached()
    with pytest.raises(ValueError):
        ix.search_rows([[1, 2]], 3)
    with pytest.raises(ValueError):
        ix.search_range_rows([1, 2], NAN, 3)
    with pytest.raises(ValueError):
        ix.search_range_rows([1, 2], [0.1, 0.2, 0.3], 3)
    with pytest.raises(ValueError):
        ix.search_range_rows_device([1, 2], [0.1], 3, 0, 0, 0)
    with pytest.raises(ValueError):
        ix.knn_graph(3, row0=5, row1=2)
    with pytest.raises(ValueError):
        ix.near_duplicates(0.1, block=0)


# ---- the service method over a stand-in ---------------------------------------------------------------------------------------

class RowsOracleIndex(OracleIndex):
    """the stand-in of tests/helpers.py, with the two row searches answered by the reference over the oracle's distances"""

    calls = []

    def search_rows(self, row_ids, k, include_self=False):
        type(self).calls.append(("search_rows", np.asarray(row_ids).tolist(), k, include_self))
        return rows_ref.search_rows(self._o, self._rows, row_ids, k, self.metric, None, include_self, self.row_offset)

    def search_range_rows(self, row_ids, radius, max_results, include_self=False):
        from autorag_research_amd.index import Mi355Index

        type(self).calls.append(("search_range_rows", np.asarray(row_ids).tolist(), max_results, include_self))
        radius = Mi355Index._radius(radius, len(row_ids))           # (the wrapper's own check: a scalar, or one per slot)
        return rows_ref.search_range_rows(self._o, self._rows, row_ids, radius, max_results, self.metric, None, include_self,
                                          self.row_offset)


@pytest.fixture()
def svc(monkeypatch, oracle):
    import autorag_research_amd.service as service

    monkeypatch.setattr(service, "Mi355Index", RowsOracleIndex)
    RowsOracleIndex.calls = []
    store, g = build_golden_stores()
    s = service.Mi355RetrievalService(lambda: store)
    yield s, g
    s.close()


def test_service_similar_chunks(svc):
    s, g = svc
    ids = list(g["ids"])
    keys = [ids[4], ids[0], ids[17], ids[4]]                        # any order, a key twice: every slot is answered
    out = s.similar_chunks(keys, top_k=6)
    assert len(out) == 4 and out[0] == out[3]
    assert RowsOracleIndex.calls == [("search_rows", [4, 0, 17, 4], 6, False)]     # key -> table position -> index row
    for pk, res in zip(keys, out):
        emb = [float(x) for x in g["C"][ids.index(pk)]]
        by_emb = s.vector_search_by_embedding(emb, 7)
        assert pk in [r["doc_id"] for r in by_emb]                  # (the chunk is its own nearest, or a tie of it)
        assert pk not in [r["doc_id"] for r in res] and len(res) == 6
        assert res == [r for r in by_emb if r["doc_id"] != pk][:6]  # dicts, contents and scores = 1 - distance
        assert all(r["content"] is not None for r in res)
    d, r = rows_ref.search_rows(s._unit("chunk").single._o, np.asarray(g["C"], dtype=np.float32), [4], 6)
    assert [x["score"] for x in out[0]] == (1.0 - d[0]).tolist() and [x["doc_id"] for x in out[0]] == [ids[i] for i in r[0]]
    assert s.similar_chunks([]) == []
    # the image unit: no contents
    img = s.similar_chunks([g["img_ids"][2]], top_k=3, unit="image_chunk")
    assert len(img[0]) == 3 and all(x["content"] is None for x in img[0]) and g["img_ids"][2] not in [x["doc_id"] for x in img[0]]


def test_service_similar_chunks_within_a_distance(svc):
    s, g = svc
    ids = list(g["ids"])
    plain = s.similar_chunks([ids[1], ids[9]], top_k=8)
    r3 = 1.0 - plain[0][2]["score"]                                 # the distance of the third neighbour admits three
    out = s.similar_chunks([ids[1], ids[9]], top_k=2, max_distance=[r3, -1.0])
    assert out[0] == (plain[0][:2], 3) and out[1] == ([], 0)
    out = s.similar_chunks([ids[1], ids[9]], top_k=8, max_distance=INF)
    assert [res for res, _ in out] == plain and [c for _, c in out] == [len(ids) - 1] * 2
    assert RowsOracleIndex.calls[-1][0] == "search_range_rows"
    with pytest.raises(ValueError):
        s.similar_chunks([ids[1], ids[9]], top_k=3, max_distance=[0.5, 0.5, 0.5])


def test_service_similar_chunks_refusals(monkeypatch, oracle):
    import autorag_research_amd.service as service
    from autorag_research_amd.store import InMemoryStore

    monkeypatch.setattr(service, "Mi355Index", RowsOracleIndex)
    RowsOracleIndex.calls = []
    rng = np.random.default_rng(5)
    emb = rng.standard_normal((6, 8)).astype(np.float32)
    emb[2] = NAN                                                    # a chunk without a stored embedding
    store = InMemoryStore()
    store.set_chunks([f"c{i}" for i in range(6)], [f"text {i}" for i in range(6)], embedding=emb)
    s = service.Mi355RetrievalService(lambda: store)
    try:
        with pytest.raises(ValueError, match="not found"):
            s.similar_chunks(["c0", "nope"])
        with pytest.raises(ValueError, match="no embedding"):
            s.similar_chunks(["c2"])
        assert RowsOracleIndex.calls == []
        # the index holds the five stored rows: c3 is row 2, and c2 is no result of anything
        out = s.similar_chunks(["c3"], top_k=10)
        assert RowsOracleIndex.calls == [("search_rows", [2], 10, False)]
        assert sorted(x["doc_id"] for x in out[0]) == ["c0", "c1", "c4", "c5"]
        s._world = object()          # a process group: refused before anything is asked of it
        with pytest.raises(NotImplementedError):
            s.similar_chunks(["c0"])
        with pytest.raises(NotImplementedError):
            s.similar_chunks(["nope"], max_distance=0.5)
    finally:
        s._world = None
        s.close()
