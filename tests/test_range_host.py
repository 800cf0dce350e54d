"""CPU: the range search's numpy restatement (tests/range_ref.py) on hand-written cases, the declaration and binding of the
two entry points, the Python wrappers' radius checks, and the two service methods over a stand-in index that answers
`search_range` from the reference."""

import re
from pathlib import Path

import numpy as np
import pytest

import range_ref
from helpers import OracleIndex, build_golden_stores

ROOT = Path(__file__).resolve().parent.parent
NAN, INF = float("nan"), float("inf")


# ---- the reference itself, by hand -----------------------------------------------------------------------------------------

def test_ref_hand_written_cases():
    #            row:  0     1     2     3    4     5
    D = np.array([[0.50, 0.25, 0.50, NAN, 0.75, 0.25],
                  [0.10, 0.20, 0.30, 0.40, 0.50, 0.60]])
    ds, rs = range_ref.sort_pairs(D)
    assert rs[0].tolist() == [1, 5, 0, 2, 4, 3] and np.isnan(ds[0, 5])         # ties by row, the NaN row last
    # a tie across the cut: rows 0 and 2 share 0.5, the lower row takes the last slot and the count holds both
    d, r, c = range_ref.search_range(ds, rs, 0.5, 3)
    assert r.tolist() == [[1, 5, 0], [0, 1, 2]] and c.tolist() == [4, 5]
    assert d[0].tolist() == [0.25, 0.25, 0.5]
    # a radius equal to a distance includes that row; the next double below it does not
    assert range_ref.search_range(ds, rs, [0.75, 0.3], 8)[2].tolist() == [5, 3]
    assert range_ref.search_range(ds, rs, np.nextafter([0.75, 0.3], -INF), 8)[2].tolist() == [4, 2]
    # +inf: every row with a distance -- never the NaN row; -inf: none; the tail is NaN / -1
    d, r, c = range_ref.search_range(ds, rs, [INF, -INF], 8)
    assert c.tolist() == [5, 0] and r[0].tolist() == [1, 5, 0, 2, 4, -1, -1, -1] and (r[1] == -1).all()
    assert np.isnan(d[0, 5:]).all() and np.isnan(d[1]).all()
    # removed rows are never in range
    live = np.array([True, False, True, True, True, True])
    d, r, c = range_ref.search_range(ds, rs, 0.5, 2, live)
    assert r.tolist() == [[5, 0], [0, 2]] and c.tolist() == [3, 4]
    # per-query radii from wanted counts
    radius, counts = range_ref.radius_admitting(ds, rs, [2, 0])
    assert radius.tolist() == [0.25, -INF] and counts.tolist() == [2, 0]
    # compared as doubles: -0.0 <= +0.0 and +0.0 <= -0.0
    z, zr = range_ref.sort_pairs(np.array([[0.0, -0.0, 1.0]]))
    assert range_ref.search_range(z, zr, -0.0, 4)[2].tolist() == [2] and range_ref.search_range(z, zr, 0.0, 4)[2].tolist() == [2]


def test_ref_equals_masked_topk(oracle):
    """the identity the header states: search at k = max_results with every entry that is NaN or above the radius blanked"""
    rng = np.random.default_rng(3)
    C = rng.standard_normal((200, 16)).astype(np.float32)
    C[7] = 0.0
    C[50] = C[51]
    Q = rng.standard_normal((5, 16)).astype(np.float32)
    for metric in ("cosine", "ip"):
        ds, rs = range_ref.oracle_sorted(oracle, C, Q, metric)
        radius, _ = range_ref.radius_admitting(ds, rs, [0, 1, 9, 10, 150])
        d, r, c = range_ref.search_range(ds, rs, radius, 10)
        td, tr = oracle.topk_search(C, Q, 10, metric=metric)
        with np.errstate(invalid="ignore"):
            out = np.isnan(td) | (td > radius[:, None])
        assert np.array_equal(r, np.where(out, -1, tr)) and np.array_equal(np.isnan(d), out)
        assert np.array_equal(d[~out].view(np.uint64), td[~out].view(np.uint64))
        assert c.tolist() == [0, 1, 9, 10, 150]


# ---- the ABI and its binding --------------------------------------------------------------------------------------------------

def test_header_declares_and_native_binds_both_entry_points(native_built):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mi355dr.h").read_text(), flags=re.S)
    for name in ("mi355dr_search_range", "mi355dr_search_range_device"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    from autorag_research_amd import _native

    assert {"mi355dr_search_range", "mi355dr_search_range_device"} <= set(_native.ABI_SYMBOLS)
    lib = _native.load()
    assert len(lib.mi355dr_search_range.argtypes) == 8 and len(lib.mi355dr_search_range_device.argtypes) == 9


def test_wrappers_refuse_a_bad_radius_before_the_library():
    from autorag_research_amd.index import Mi355Index

    assert Mi355Index._radius(0.25, 3).tolist() == [0.25] * 3
    assert Mi355Index._radius([0.1, INF, -INF], 3).tolist() == [0.1, INF, -INF]
    assert Mi355Index._radius(np.float32(0.5), 1).dtype == np.float64
    for bad, B in ((NAN, 2), ([0.1, NAN], 2), ([0.1, 0.2, 0.3], 2), ([[0.1, 0.2]], 2), ([], 1)):
        with pytest.raises(ValueError):
            Mi355Index._radius(bad, B)

    class Unreached(Mi355Index):   # (no handle: the checks come before the first use of the library)
        def __init__(self):
            self.dim = 4

        def __del__(self):
            pass

    ix = Unreached()
    with pytest.raises(ValueError):
        ix.search_range(np.zeros((2, 4), np.float32), NAN, 3)
    with pytest.raises(ValueError):
        ix.search_range(np.zeros((2, 4), np.float32), [0.1, 0.2, 0.3], 3)
    with pytest.raises(ValueError):
        ix.search_range_device(0, 2, [0.1], 3, 0, 0, 0)


# ---- the service methods over a stand-in --------------------------------------------------------------------------------------

class RangeOracleIndex(OracleIndex):
    """the stand-in of tests/helpers.py, with `search_range` answered by the reference over the oracle's distances"""

    def search_range(self, queries, radius, max_results):
        from autorag_research_amd.index import Mi355Index

        q = np.ascontiguousarray(queries, dtype=np.float32)
        q = q[None, :] if q.ndim == 1 else q
        ds, rs = range_ref.oracle_sorted(self._o, self._rows, q, self.metric)
        d, r, c = range_ref.search_range(ds, rs, Mi355Index._radius(radius, q.shape[0]), max_results)
        return d, np.where(r >= 0, r + self.row_offset, r), c


@pytest.fixture()
def svc(monkeypatch, oracle):
    import autorag_research_amd.service as service

    monkeypatch.setattr(service, "Mi355Index", RangeOracleIndex)
    store, g = build_golden_stores()
    s = service.Mi355RetrievalService(lambda: store)
    yield s, g
    s.close()


def test_service_range_by_embedding(svc):
    s, g = svc
    emb = [float(x) for x in g["Q"][2]]
    top = s.vector_search_by_embedding(emb, 12)
    assert len(top) == 12 and len({r["score"] for r in top}) == 12
    n = len(g["ids"])
    # everything is within +inf: the ordinary results (ids, contents, scores), the count is the whole table
    res, count = s.vector_search_range_by_embedding(emb, INF, limit=12)
    assert res == top and count == n
    # the distance of the 5th result admits exactly five: id mapping and score conversion as `vector_search_by_embedding`
    r5 = 1.0 - top[4]["score"]
    res, count = s.vector_search_range_by_embedding(emb, r5, limit=10)
    assert res == top[:5] and count == 5 and all(r["content"] is not None for r in res)
    # count > limit: the list is cut, the count is not
    res, count = s.vector_search_range_by_embedding(emb, r5, limit=2)
    assert res == top[:2] and count == 5
    # nothing within the distance; no embedding
    assert s.vector_search_range_by_embedding(emb, -1.0) == ([], 0)
    assert s.vector_search_range_by_embedding([], 0.5) == ([], 0)
    # the image unit: no contents
    res, count = s.vector_search_range_by_embedding(emb, r5, limit=10, unit="image_chunk")
    assert [r["score"] for r in res] == [r["score"] for r in top[:5]] and all(r["content"] is None for r in res) and count == 5


def test_service_range_by_query_ids(svc):
    s, g = svc
    qids = [f"q{i}" for i in range(6)]
    tops = s.vector_search(qids, 8)
    radii = [1.0 - tops[i][i]["score"] for i in range(6)]          # query i admits i + 1 chunks
    out = s.vector_search_range(qids, radii, limit=4)
    assert [c for _, c in out] == [1, 2, 3, 4, 5, 6]
    assert [res for res, _ in out] == [tops[i][:min(i + 1, 4)] for i in range(6)]
    # a scalar distance for all; one query equals the by-embedding form
    out = s.vector_search_range(qids, 0.8, limit=3)
    for i, (res, count) in enumerate(out):
        assert (res, count) == s.vector_search_range_by_embedding([float(x) for x in g["Q"][i]], 0.8, limit=3)
    assert s.vector_search_range([], 0.5) == []
    with pytest.raises(ValueError, match="not found"):
        s.vector_search_range(["nope"], 0.5)
    with pytest.raises(ValueError, match="no embedding"):
        s.vector_search_range(["q_noemb"], 0.5)
    with pytest.raises(ValueError):
        s.vector_search_range(qids, [0.5, 0.5], limit=3)            # one radius per query, or one for all
