"""CPU reference of the MMR search (include/mi355dr.h "MMR search"), in plain Python floats -- IEEE double, one operation
per line of the definition, nothing fused -- over the oracle's `topk_search`, `cosine_distance` and `dot`.

Candidate order: the library's total order (distance asc, NaN last, row asc).  Eligible candidates: the leading entries with
row >= 0 and a non-NaN distance.  sim(dist) = 1.0 - dist (cosine), -dist (inner product).  pairdist(a, b) = the oracle's exact
distance of the two stored rows: `cosine_distance(C[a], C[b])` / `-dot(C[a], C[b])`.

    sq[i]  = sim(dist[i])
    one_m  = 1.0 - lambda
    pick 0 = candidate 0
    after each pick c, except the last, for every unselected i:
        s = sim(pairdist(c, i));  ms[i] = s at the first pick;  ms[i] = s if s > ms[i] afterwards (a NaN s is ignored)
    pick t >= 1: score[i] = lambda * sq[i] - one_m * ms[i] over the unselected i; the first i whose score is strictly greater
        than every earlier unselected score; a NaN score never wins; if none wins, the first unselected i

Stop after min(k, n) picks; slot t = pick t's query distance (unchanged) and global row; the rest NaN / -1."""

import math

import numpy as np


def sim(metric, dist):
    return 1.0 - dist if metric == "cosine" else -dist


def pairdist_scalar(oracle, C, a, others, metric):
    """pairdist(a, i) for i in others, one oracle call per pair: the definition"""
    if metric == "cosine":
        return [oracle.cosine_distance(C[a], C[i]) for i in others]
    return [-oracle.dot(C[a], C[i]) for i in others]


def pairdist_batched(oracle, C, a, others, metric):
    """the same numbers from ONE `topk_search` of the row C[a] as the query over the rows `others` (every row returned, mapped
    back by position): the oracle's distance is symmetric in its two vectors, and this is what keeps k = fetch_k = 1024 quick"""
    others = list(others)
    if not others:
        return []
    d, r = oracle.topk_search(C[others], C[a], len(others), metric=metric, threads=1)
    out = [math.nan] * len(others)
    for x, j in zip(d[0].tolist(), r[0].tolist()):
        if j >= 0:
            out[j] = x
    return out


def mmr_pick(oracle, C, dist, rows, k, lam, metric="cosine", pairdist=pairdist_batched):
    """One query.  dist / rows: its candidate list in the total order, rows LOCAL (indices into C; -1 = none).
    Returns (positions picked, in pick order; number of (picked, candidate) pairs scored)."""
    dist = [float(x) for x in dist]
    rows = [int(x) for x in rows]
    n = 0
    while n < len(rows) and rows[n] >= 0 and not math.isnan(dist[n]):
        n += 1
    picks = min(k, n)
    if picks == 0:
        return [], 0
    sq = [sim(metric, dist[i]) for i in range(n)]
    one_m = 1.0 - lam
    ms = [None] * n
    selected = [False] * n
    order, pairs, cur = [], 0, 0
    for t in range(picks):
        if t >= 1:
            best, best_score = None, None
            for i in range(n):
                if selected[i]:
                    continue
                a = lam * sq[i]
                b = one_m * ms[i]
                score = a - b
                if score != score:
                    continue
                if best is None or score > best_score:
                    best, best_score = i, score
            cur = best if best is not None else selected.index(False)
        selected[cur] = True
        order.append(cur)
        if t == picks - 1:
            break
        todo = [i for i in range(n) if not selected[i]]
        for i, pd in zip(todo, pairdist(oracle, C, rows[cur], [rows[i] for i in todo], metric)):
            s = sim(metric, pd)
            if t == 0:
                ms[i] = s
            elif s > ms[i]:
                ms[i] = s
        pairs += len(todo)
    return order, pairs


def mmr_from_lists(oracle, C, dist, rows, k, lam, metric="cosine", row_offset=0, pairdist=pairdist_batched):
    """dist / rows [B, f]: every query's candidate list in the total order, rows as the library returns them (global = index
    into C + row_offset; -1 = none).
    Returns (distance float64 [B, k], rows int64 [B, k], pairs scored)."""
    dist, rows = np.asarray(dist, dtype=np.float64), np.asarray(rows, dtype=np.int64)
    B = dist.shape[0]
    out_d, out_r, pairs = np.full((B, k), np.nan), np.full((B, k), -1, dtype=np.int64), 0
    for b in range(B):
        local = np.where(rows[b] >= 0, rows[b] - row_offset, -1)
        order, p = mmr_pick(oracle, C, dist[b], local, k, lam, metric, pairdist)
        pairs += p
        for t, i in enumerate(order):
            out_d[b, t], out_r[b, t] = dist[b, i], rows[b, i]
    return out_d, out_r, pairs


def search_mmr(oracle, C, Q, k, fetch_k, lam, metric="cosine", row_offset=0, pairdist=pairdist_batched):
    """the reference of Mi355Index.search_mmr over the corpus C (local row = index into C)"""
    d, r = oracle.topk_search(C, Q, fetch_k, metric=metric)
    return mmr_from_lists(oracle, C, d, np.where(r >= 0, r + row_offset, -1), k, lam, metric, row_offset, pairdist)


def mmr_select(oracle, C, Q, k, cand_rows, lam, metric="cosine", row_offset=0, live=None, pairdist=pairdist_batched):
    """the reference of Mi355Index.mmr_select: each query's own pool (global ids; ids outside C and -1 skipped, duplicates
    once, rows not in `live` skipped), ordered as the restricted search orders it -- `topk_search` over the sorted unique rows,
    positions mapped back -- then picked from"""
    Q = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, C.shape[1])
    cand_rows = np.asarray(cand_rows, dtype=np.int64).reshape(Q.shape[0], -1)
    m = cand_rows.shape[1]
    dist, rows = np.full((Q.shape[0], max(m, 1)), np.nan), np.full((Q.shape[0], max(m, 1)), -1, dtype=np.int64)
    for b in range(Q.shape[0]):
        ids = np.unique(cand_rows[b] - row_offset)
        ids = ids[(ids >= 0) & (ids < C.shape[0])]
        if live is not None:
            ids = ids[live[ids]]
        if ids.size == 0:
            continue
        d, r = oracle.topk_search(C[ids], Q[b], ids.size, metric=metric, threads=1)
        dist[b, :ids.size] = d[0]
        rows[b, :ids.size] = np.where(r[0] >= 0, ids[np.maximum(r[0], 0)] + row_offset, -1)
    return mmr_from_lists(oracle, C, dist, rows, k, lam, metric, row_offset, pairdist)


# ---- the corpora of the MMR tests -----------------------------------------------------------------------------------------
_CORPORA = {}


def clustered(d, B=5):
    """200 Gaussian centres x 10 near-copies (+ 0.05 noise), shuffled; queries = a centre + 0.3 noise: the ten nearest rows of
    a query are near-copies of each other, so MMR at lambda = 0.5 leaves the plain top-k"""
    if ("c", d, B) not in _CORPORA:
        rng = np.random.default_rng(7)
        centres = rng.standard_normal((200, d))
        C = np.repeat(centres, 10, axis=0) + 0.05 * rng.standard_normal((2000, d))
        C = C[rng.permutation(2000)].astype(np.float32)
        Q = (centres[rng.choice(200, size=B, replace=False)] + 0.3 * rng.standard_normal((B, d))).astype(np.float32)
        _CORPORA[("c", d, B)] = (C, Q)
    return _CORPORA[("c", d, B)]


def gaussian(d, B=5, n=2000):
    if ("g", d, B, n) not in _CORPORA:
        rng = np.random.default_rng([7, d, n])
        _CORPORA[("g", d, B, n)] = (rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((B, d)).astype(np.float32))
    return _CORPORA[("g", d, B, n)]


def same(a, b):
    """two (dist, rows) results agree bit for bit (NaN positions, not payloads)"""
    (da, ra), (db, rb) = a[:2], b[:2]
    assert np.array_equal(ra, rb)
    assert np.array_equal(np.isnan(da), np.isnan(db))
    ok = ~np.isnan(da)
    assert np.array_equal(np.ascontiguousarray(da[ok]).view(np.uint64), np.ascontiguousarray(db[ok]).view(np.uint64))
