"""CPU reference of the search by examples and of Rocchio feedback (include/mi355dr.h "search by examples / feedback"),
restated in numpy for the tests.

The combination is written in float64 element-wise, one operation per line of the rule, so that every rounding is the
rule's; the norms are the oracle's (`row_nrm2`: the k-ascending fp32 chain) and so are all distances:
    s(v)  = 1.0 / sqrt((double)nrm2(v))   cosine          s(v) = 1.0   inner product
    cp    = beta / (valid positives)      cn = gamma / (valid negatives)
    acc   = alpha * (s(q) * q_i);  acc = acc + cp * (s_j * c_ji) per valid positive in list order;
            acc = acc - cn * (s_j * c_ji) per valid negative in list order;  q'_i = (float)acc
A listed position is valid iff its id is a live row of the shard whose stored squared norm is finite and > 0; a base iff its
squared norm is; a slot is invalid with an invalid base or without any valid term.
"""

import numpy as np


def ids_2d(ids, B):
    """ragged lists / an array / None -> int64 [B, m], -1 padded"""
    if ids is None:
        return np.full((B, 0), -1, dtype=np.int64)
    if isinstance(ids, np.ndarray) and ids.ndim == 2:
        assert ids.shape[0] == B
        return ids.astype(np.int64)
    ids = [np.asarray(x, dtype=np.int64).reshape(-1) for x in ids]
    assert len(ids) == B
    out = np.full((B, max((len(x) for x in ids), default=0)), -1, dtype=np.int64)
    for b, x in enumerate(ids):
        out[b, :len(x)] = x
    return out


def _scale(n2, metric):
    if metric != "cosine":
        return np.float64(1.0)
    root = np.sqrt(np.float64(n2))
    return np.float64(1.0) / root


def _norm_ok(n2):
    return bool(np.isfinite(n2) and n2 > 0)


def combine(oracle, C, Q, pos, neg, alpha, beta, gamma, metric="cosine", row_offset=0, live=None, listed=None):
    """-> (q' float32 [B, d], valid int32 [B], stats {"skipped", "skipped_slots"}).  Q: [B, d] or None.  `listed`: bool
    [B, mp] -- positions of `pos` that are positions at all (the feedback form: a list's padding and NaN entries are none);
    default: every position."""
    C = np.ascontiguousarray(C, dtype=np.float32)
    n, d = C.shape
    B = len(Q) if Q is not None else len(pos)
    pos, neg = ids_2d(pos, B), ids_2d(neg, B)
    nrm2 = oracle.row_nrm2(C) if n else np.zeros(0, dtype=np.float32)
    alive = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    alpha, beta, gamma = np.float64(alpha), np.float64(beta), np.float64(gamma)
    out = np.zeros((B, d), dtype=np.float32)
    valid = np.zeros(B, dtype=np.int32)
    stats = {"skipped": 0, "skipped_slots": 0}

    def examples(ids, mask):
        got = []
        for j, gid in enumerate(ids.tolist()):
            if mask is not None and not mask[j]:
                continue
            r = gid - int(row_offset)
            if 0 <= r < n and alive[r] and _norm_ok(nrm2[r]):
                got.append((r, _scale(nrm2[r], metric)))
            else:
                stats["skipped"] += 1
        return got

    with np.errstate(all="ignore"):
        for b in range(B):
            vp = examples(pos[b], None if listed is None else listed[b])
            vn = examples(neg[b], None)
            base_ok = False
            if Q is not None:
                q = np.ascontiguousarray(Q[b], dtype=np.float32)
                nq = oracle.row_nrm2(q[None, :])[0]
                base_ok = _norm_ok(nq)
            if (Q is not None and not base_ok) or (Q is None and not vp and not vn):
                stats["skipped_slots"] += 1
                continue
            acc = np.zeros(d, dtype=np.float64)
            if Q is not None:
                t = q.astype(np.float64)
                t = _scale(nq, metric) * t
                acc = alpha * t
            if vp:
                cp = beta / np.float64(len(vp))
                for r, s in vp:
                    t = C[r].astype(np.float64)
                    t = s * t
                    t = cp * t
                    acc = acc + t
            if vn:
                cn = gamma / np.float64(len(vn))
                for r, s in vn:
                    t = C[r].astype(np.float64)
                    t = s * t
                    t = cn * t
                    acc = acc - t
            out[b] = acc.astype(np.float32)
            valid[b] = 1
    return out, valid, stats


def _ranking(oracle, C, Qp, depth, metric, live):
    """the oracle's total order of Qp against C, deep enough that `depth` live rows are in it (or the order has ended), the
    removed rows taken out: a list of (dist [..], local rows [..]) per query"""
    n = len(C)
    alive = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    deep = min(n, depth + int((~alive).sum()))
    if len(Qp) == 0 or deep == 0:
        return [(np.zeros(0), np.zeros(0, dtype=np.int64)) for _ in range(len(Qp))]
    ds, rs = oracle.topk_search(C, np.ascontiguousarray(Qp, dtype=np.float32), deep, metric=metric)
    out = []
    for i in range(len(Qp)):
        keep = rs[i] >= 0
        keep &= alive[np.maximum(rs[i], 0)]
        out.append((ds[i, keep], rs[i, keep]))
    return out


def _blank(B, k):
    return np.full((B, k), np.nan, dtype=np.float64), np.full((B, k), -1, dtype=np.int64)


def search_examples(oracle, C, Q, pos, neg, alpha, beta, gamma, k, metric="cosine", row_offset=0, live=None, keep=False):
    """-> (dist float64 [B, k], rows int64 [B, k] global, stats).  The ranking of q' at k + mp + mn live rows, then the strike
    in plain Python: every listed id goes, the first k survivors stay."""
    C = np.ascontiguousarray(C, dtype=np.float32)
    B = len(Q) if Q is not None else len(pos)
    pos, neg = ids_2d(pos, B), ids_2d(neg, B)
    qp, valid, stats = combine(oracle, C, Q, pos, neg, alpha, beta, gamma, metric, row_offset, live)
    dist, rows = _blank(B, k)
    at = np.flatnonzero(valid)
    depth = k if keep else k + pos.shape[1] + neg.shape[1]
    for b, (ds, rs) in zip(at, _ranking(oracle, C, qp[at], depth, metric, live)):
        struck = set() if keep else set(pos[b].tolist()) | set(neg[b].tolist())
        j = 0
        for dv, r in zip(ds[:depth].tolist(), rs[:depth].tolist()):
            if r + int(row_offset) in struck:
                continue
            if j == k:
                break
            dist[b, j], rows[b, j] = dv, r + int(row_offset)
            j += 1
    return dist, rows, stats


def search_plain(oracle, C, Q, k, metric="cosine", row_offset=0, live=None):
    """the ordinary search over the live rows: (dist [B, k], rows [B, k] global), NaN / -1 padded"""
    C = np.ascontiguousarray(C, dtype=np.float32)
    dist, rows = _blank(len(Q), k)
    for b, (ds, rs) in enumerate(_ranking(oracle, C, Q, k, metric, live)):
        m = min(k, len(rs))
        dist[b, :m], rows[b, :m] = ds[:m], rs[:m] + int(row_offset)
    return dist, rows


def search_feedback(oracle, C, Q, k, fb_k, alpha, beta, metric="cosine", row_offset=0, live=None):
    """-> (dist, rows, stats, q').  Pass 1 at fb_k; its entries with a row and a non-NaN distance are the positives, in list
    order; q' from alpha, beta and the query as base; pass 2 at k, nothing struck; an invalid slot blanked."""
    C = np.ascontiguousarray(C, dtype=np.float32)
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    d1, r1 = search_plain(oracle, C, Q, fb_k, metric, row_offset, live)
    listed = (r1 >= 0) & ~np.isnan(d1)
    qp, valid, stats = combine(oracle, C, Q, r1, None, alpha, beta, 0.0, metric, row_offset, live, listed=listed)
    dist, rows = _blank(len(Q), k)
    at = np.flatnonzero(valid)
    if len(at):
        dist[at], rows[at] = search_plain(oracle, C, qp[at], k, metric, row_offset, live)
    return dist, rows, stats, qp


def clustered(n, d, n_clusters, seed, spread=0.35):
    """n rows around n_clusters unit centres (the corpus shape of mmr_ref.clustered): a query near the edge of a cluster is
    pulled into it by feedback, so the second pass differs from the first"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, d))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    which = rng.integers(0, n_clusters, size=n)
    C = centres[which] + spread * rng.standard_normal((n, d)) / np.sqrt(d)
    return np.ascontiguousarray(C, dtype=np.float32), centres.astype(np.float32)


N_BASE = 1000


def base_rows(d, seed=0):
    """the 1000-row corpus of tests/test_gpu_rows.py (a multiple of neither 32 nor 128) with every row class; components stay
    out of the fp32 denormal range"""
    rng = np.random.default_rng(1000 * d + seed)
    C = rng.standard_normal((N_BASE, d)).astype(np.float32)
    C *= rng.uniform(0.5, 2.0, size=(N_BASE, 1)).astype(np.float32)
    C[5] = 0.0                                  # zero row: NaN under cosine, distance -0.0 under inner product
    C[17, 2] = np.nan                           # rows with non-finite components
    C[18, 4] = np.inf
    C[19] *= 1e20                               # huge norm: |c|^2 overflows
    C[9, 3] = 40.0 * np.abs(C[9]).max()         # one dominant component: loose under the int8 screen
    C[611, 7] = -60.0 * np.abs(C[611]).max()
    C[300] = C[301] = C[302] = C[40]            # duplicates: equal distance bits, the row decides
    C.setflags(write=False)
    return C


# the feedback cases of tests/test_gpu_examples.py: (name, metric, d, rows, queries, k, fb_k, alpha, beta).  Clustered corpora
# (tests/test_examples_ref.py checks that every case's expectation differs from the plain search for some query)
FEEDBACK_CASES = [
    ("cosine", "cosine", 70, 1000, 12, 10, 10, 1.0, 0.75),
    ("ip", "ip", 70, 1000, 12, 10, 10, 1.0, 0.75),
    ("d768", "cosine", 768, 600, 9, 5, 8, 1.0, 1.0),
    ("short", "cosine", 70, 300, 7, 10, 400, 0.5, 1.0),      # fb_k above the live rows: fewer positives than fb_k
    ("deep", "cosine", 70, 1500, 5, 32, 1024, 1.0, 4.0),     # fb_k = 1024
]


def feedback_case(name):
    """-> (C, Q, metric, k, fb_k, alpha, beta): a clustered corpus and queries between two of its clusters"""
    _, metric, d, n, B, k, fb_k, alpha, beta = next(c for c in FEEDBACK_CASES if c[0] == name)
    seed = 7000 + [c[0] for c in FEEDBACK_CASES].index(name)
    C, centres = clustered(n, d, 12, seed)
    rng = np.random.default_rng(seed + 1)
    a, b = rng.integers(0, 12, size=B), rng.integers(0, 12, size=B)
    w = rng.uniform(0.5, 0.6, size=(B, 1))
    Q = w * centres[a] + (1.0 - w) * centres[b] + 0.3 * rng.standard_normal((B, d)) / np.sqrt(d)
    C.setflags(write=False)
    return C, np.ascontiguousarray(Q, dtype=np.float32), metric, k, fb_k, alpha, beta


def same_lists(got, exp):
    """all distances bit for bit (NaN where NaN) and all rows"""
    (gd, gr), (ed, er) = got[:2], exp[:2]
    assert gd.shape == ed.shape and gr.shape == er.shape
    assert np.array_equal(gr, er), f"rows differ in slots {np.flatnonzero((gr != er).any(axis=1))[:8]}"
    nan = np.isnan(ed)
    assert np.array_equal(np.isnan(gd), nan)
    assert np.array_equal(gd[~nan].view(np.uint64), ed[~nan].view(np.uint64))
