"""CPU reference of the hybrid fusion (include/mi355dr.h "hybrid fusion") for the tests, and the inputs they share.

An entry is struck out by the header's rule (id < 0, NaN value, id outside its map or mapped below 0) and its value becomes a
score in numpy float64 (`1.0 - v`, `-v`, `v`).  The surviving entries become the result dicts the pipelines build, and RRF,
`mm` and `tmm` are then computed by the project's own host code -- `hybrid.rrf_fuse` / `hybrid.cc_fuse`, which
tests/test_host_logic.py pins to the reference's fixtures.  `z` and `dbsf` restate the header with explicit left-to-right loops
and `math.sqrt`: `hybrid._mean_std` takes the root as `** 0.5` and sums with `sum()`, which is compensated from Python 3.12
on, so it is not what the header fixes (tests/test_fuse_ref.py shows where the two agree).
"""

import math

import numpy as np

from autorag_research_amd.hybrid import MISSING_SCORE_FLOORS, cc_fuse, rrf_fuse

METHODS = ("rrf", "mm", "tmm", "z", "dbsf")


def entries(vals, ids, mode, id_map=None):
    """One query's list -> [{"doc_id": common id, "score": float}] in list order, struck-out slots dropped."""
    vals = np.asarray(vals, dtype=np.float64)
    score = {"one_minus": 1.0 - vals, "negate": -vals, "as_is": vals}[mode].tolist()
    out = []
    for v, s, i in zip(vals.tolist(), score, np.asarray(ids, dtype=np.int64).tolist()):
        if i < 0 or v != v:
            continue
        if id_map is not None:
            if i >= len(id_map) or id_map[i] < 0:
                continue
            i = int(id_map[i])
        out.append({"doc_id": i, "score": s})
    return out


def columns(results_1, results_2):
    """(union ids in first-seen order, column 1, column 2) with None for an absent score: cc_fuse's own first lines."""
    raw_1 = {r["doc_id"]: r["score"] for r in results_1}
    raw_2 = {r["doc_id"]: r["score"] for r in results_2}
    ids = list(raw_1) + [pk for pk in raw_2 if pk not in raw_1]
    return ids, [raw_1.get(pk) for pk in ids], [raw_2.get(pk) for pk in ids]


def mean_std(live):
    """The header's statistics: two plain left-to-right sums from 0.0 and the correctly rounded root."""
    n = len(live)
    total = 0.0
    for s in live:
        total = total + s
    mean = total / float(n)
    acc = 0.0
    for s in live:
        acc = acc + (s - mean) * (s - mean)
    var = acc / float(n)
    return mean, math.sqrt(var), var


def _normalise(col, method):
    live = [s for s in col if s is not None]
    if not live:
        return list(col)
    mean, std, _ = mean_std(live)
    if method == "z":
        return [None if s is None else (0.0 if std == 0 else (s - mean) / std) for s in col]
    if std == 0:
        return [None if s is None else 0.5 for s in col]
    lo = mean - 3.0 * std
    span = (mean + 3.0 * std) - lo
    out = []
    for s in col:
        if s is None:
            out.append(None)
            continue
        x = (s - lo) / span
        y = x if x < 1.0 else 1.0
        out.append(y if y > 0.0 else 0.0)
    return out


def cc_restated(results_1, results_2, weight, method):
    """`z` / `dbsf` by the header: every document of the union with its f, sorted (f desc, first-seen order)."""
    ids, col_1, col_2 = columns(results_1, results_2)
    n1, n2, floor = _normalise(col_1, method), _normalise(col_2, method), MISSING_SCORE_FLOORS[method]
    fused = [(pk, (weight * (floor if a is None else a)) + ((1.0 - weight) * (floor if b is None else b)))
             for pk, a, b in zip(ids, n1, n2)]
    ranked = sorted(fused, key=lambda item: item[1], reverse=True)
    return [{"doc_id": pk, "score": f} for pk, f in ranked]


def fuse_query(results_1, results_2, method, rrf_k=60, fetch_k=0, weight=0.5, mins=None):
    """The whole fused union of one query as result dicts."""
    everything = len(results_1) + len(results_2)
    if method == "rrf":
        return rrf_fuse(results_1, results_2, rrf_k, everything, fetch_k)
    if method in ("mm", "tmm"):
        lo = mins if method == "tmm" else (None, None)
        return cc_fuse(results_1, results_2, weight, everything, method, lo[0], lo[1])
    return cc_restated(results_1, results_2, weight, method)


def fuse_lists(vals1, ids1, vals2, ids2, k, *, method, modes=("as_is", "as_is"), rrf_k=60, fetch_k=0, weight=0.5, mins=None,
               map1=None, map2=None):
    """What Mi355Index.fuse_lists returns: (scores float64 [B,k], ids int64 [B,k], count int32 [B]), NaN / -1 padded."""
    B = len(vals1)
    out_v = np.full((B, k), np.nan)
    out_i = np.full((B, k), -1, dtype=np.int64)
    count = np.zeros(B, dtype=np.int32)
    for q in range(B):
        fused = fuse_query(entries(vals1[q], ids1[q], modes[0], map1), entries(vals2[q], ids2[q], modes[1], map2), method,
                           rrf_k, fetch_k, weight, mins)
        count[q] = len(fused)
        for j, r in enumerate(fused[:k]):
            out_v[q, j], out_i[q, j] = r["score"], r["doc_id"]
    return out_v, out_i, count


def same(got, want):
    """ids equal, scores equal AS BITS (a NaN by position), counts equal"""
    (gv, gi, gc), (wv, wi, wc) = got, want
    assert gv.shape == wv.shape and gi.shape == wi.shape
    assert np.array_equal(gi, wi)
    assert np.array_equal(np.isnan(gv), np.isnan(wv))
    ok = ~np.isnan(wv)
    assert np.array_equal(np.ascontiguousarray(gv[ok]).view(np.uint64), np.ascontiguousarray(wv[ok]).view(np.uint64))
    assert np.array_equal(np.asarray(gc, dtype=np.int64), np.asarray(wc, dtype=np.int64))


# ---- the inputs tests/test_gpu_fuse.py runs and tests/test_fuse_ref.py checks the z / dbsf restatement on ------------------------

SHAPES = ((1, 1), (3, 5), (64, 64), (65, 63), (1024, 1024), (1, 1024))
OVERLAPS = ("identical", "disjoint", "half", "random")


def make_lists(seed, B, w1, w2, overlap="random", tails=(0, 0), holes=False, equal=()):
    """Two lists per query over a small id universe.  `overlap`: list 2 repeats list 1's ids ("identical", as far as it is
    long), shares none ("disjoint"), shares its first half with list 1 in the OPPOSITE order ("half"), or is drawn
    independently ("random").  Values are distances in rank order with some exact repeats.  `tails`: that many (-1, NaN) slots
    at the end of each list, per query one fewer down to none; `holes`: an id of -1 beside a number and a NaN beside an id in
    the middle of both lists; `equal`: the lists (0 / 1) whose values are all one number."""
    rng = np.random.default_rng(seed)
    universe = 3 * (w1 + w2) + 5
    vals, ids = [], []
    for w in (w1, w2):
        v = np.sort(np.round(rng.random((B, w)) * 2.0, 3), axis=1)   # (three decimals: equal neighbours happen)
        vals.append(v)
        ids.append(np.zeros((B, w), dtype=np.int64))
    for q in range(B):
        perm = rng.permutation(universe)
        ids[0][q] = perm[:w1]
        rest = perm[w1:]
        if overlap == "identical":
            shared = min(w1, w2)
            ids[1][q] = np.concatenate([ids[0][q][:shared], rest[:w2 - shared]])
        elif overlap == "disjoint":
            ids[1][q] = rest[:w2]
        elif overlap == "half":
            shared = min(w1, w2 // 2)
            ids[1][q] = np.concatenate([ids[0][q][:shared][::-1], rest[:w2 - shared]])
        else:
            ids[1][q] = rng.permutation(universe)[:w2]
    for l in equal:
        vals[l][:] = 0.625
    for l, w in enumerate((w1, w2)):
        for q in range(B):
            t = min(max(tails[l] - q, 0), w)
            if t:
                vals[l][q, w - t:], ids[l][q, w - t:] = np.nan, -1
        if holes and w >= 4:
            ids[l][:, w // 2] = -1           # a number without an id: ranks skip it
            vals[l][:, w // 2 - 1] = np.nan  # an id without a number: the same
    return vals[0], ids[0], vals[1], ids[1]


def shape_cases():
    """(name, lists) for every shape x overlap, three queries each, plus the edge lists at small shapes."""
    out = []
    for s, (w1, w2) in enumerate(SHAPES):
        for o, overlap in enumerate(OVERLAPS):
            out.append((f"{w1}x{w2}-{overlap}", make_lists(100 + 10 * s + o, 3, w1, w2, overlap)))
    out.append(("tails", make_lists(201, 4, 9, 12, "half", tails=(3, 5))))
    out.append(("holes", make_lists(202, 3, 12, 9, "half", tails=(2, 0), holes=True)))
    out.append(("holes-64", make_lists(203, 3, 65, 63, "random", tails=(1, 7), holes=True)))
    out.append(("list1-empty", make_lists(204, 2, 6, 8, "random", tails=(8, 0))))       # (tails shrink per query: q0 is empty)
    out.append(("list2-empty", make_lists(205, 2, 6, 8, "random", tails=(0, 9))))
    out.append(("both-empty", make_lists(206, 2, 6, 8, "random", tails=(7, 9))))
    out.append(("equal-1", make_lists(207, 3, 7, 9, "half", equal=(0,))))
    out.append(("equal-both", make_lists(208, 3, 7, 9, "random", equal=(0, 1))))
    out.append(("one-entry-column", make_lists(209, 3, 1, 6, "disjoint")))
    out.append(("one-entry-shared", make_lists(210, 3, 1, 6, "identical")))
    return out


def map_case(seed=301, B=3, w1=12, w2=9):
    """A non-identity map for list 1: its ids are rows of an index that holds only some of the documents.  The map is
    shorter than the largest row (an id beyond map_len) and holds a -1 (a row without a document); list 2 names documents
    directly.  Several of list 1's documents are in list 2 as well."""
    rng = np.random.default_rng(seed)
    n_docs, n_rows = 40, 30
    row_doc = rng.permutation(n_docs)[:n_rows].astype(np.int64)   # row -> document, not the identity
    row_doc[7] = -1
    id_map = row_doc[:n_rows - 4]                                 # rows n_rows - 4 ... are beyond the map
    v1 = np.sort(rng.random((B, w1)), axis=1)
    v2 = np.sort(rng.random((B, w2)) * -9.0, axis=1)
    others = np.array([r for r in range(n_rows) if r not in (7, n_rows - 2)])
    i1 = np.stack([rng.permutation(others)[:w1] for _ in range(B)]).astype(np.int64)
    i1[:, 3] = 7                                                  # (every query meets the -1 ...
    i1[:, 5] = n_rows - 2                                         #  ... and a row beyond the map; no id twice in a list)
    i2 = np.zeros((B, w2), dtype=np.int64)
    for q in range(B):
        shared = [int(id_map[r]) for r in i1[q, :4] if r < len(id_map) and id_map[r] >= 0]
        rest = [d for d in rng.permutation(n_docs).tolist() if d not in shared]
        i2[q] = (shared[::-1] + rest)[:w2]
    return (v1, i1, v2, i2), id_map


DEFAULT_KW = {"modes": ("one_minus", "negate"), "weight": 0.3, "mins": (-1.0, 0.0), "rrf_k": 60}


def all_inputs():
    """Every input the GPU tests fuse, as (name, (vals1, ids1, vals2, ids2), keywords without `method` and `fetch_k`)."""
    out = [(name, lists, dict(DEFAULT_KW)) for name, lists in shape_cases()]
    small, mid = make_lists(211, 3, 3, 5, "half"), make_lists(212, 3, 65, 63, "random", tails=(2, 0))
    for tag, lists in (("3x5", small), ("65x63", mid)):
        out.append((f"{tag}-as-is", lists, {**DEFAULT_KW, "modes": ("as_is", "as_is")}))
        out.append((f"{tag}-swapped-modes", lists, {**DEFAULT_KW, "modes": ("negate", "one_minus"), "mins": (0.0, -1.0)}))
        out.append((f"{tag}-weight-0", lists, {**DEFAULT_KW, "weight": 0.0}))
        out.append((f"{tag}-weight-1", lists, {**DEFAULT_KW, "weight": 1.0, "rrf_k": 0}))
    out.append(("zeros", (np.zeros((2, 4)), np.array([[1, 2, 3, 4]] * 2), -np.zeros((2, 3)), np.array([[3, 9, 1]] * 2)),
                {**DEFAULT_KW, "modes": ("as_is", "negate"), "weight": 1.0, "mins": (0.0, 0.0)}))   # (signed zeros)
    lists, id_map = map_case()
    out.append(("map-1", lists, {**DEFAULT_KW, "map1": id_map}))
    out.append(("map-identity", lists, {**DEFAULT_KW, "map1": np.arange(40, dtype=np.int64), "map2": np.arange(40, dtype=np.int64)}))
    out.append(("map-2", (lists[2], lists[3], lists[0], lists[1]),
                {**DEFAULT_KW, "modes": ("negate", "one_minus"), "map2": id_map}))
    out.append(("B1", make_lists(213, 1, 9, 7, "half", tails=(1, 2)), dict(DEFAULT_KW)))
    out.append(("B1030", make_lists(214, 1030, 3, 5, "random", tails=(2, 1)), dict(DEFAULT_KW)))
    return out
