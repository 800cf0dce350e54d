"""Float64 NumPy reference of the MaxSim bf16 screen (test_gpu_maxsim_screen_values.py); imports nothing of the package under test.

    T_ref(query, doc) = -sum_i max_j <bf16(q_i), bf16(d_j)>      what the screen kernels compute, without their fp32 rounding
    S(query, doc)     = -sum_i max_j <q_i, d_j>                  the same sum of the fp32 inputs
    E_ref(query)      the bound |T - S| <= E of csrc/mi355dr_maxsim.hip, from NumPy norms over the whole store
    tol(query, doc)   what fp32 accumulation may move T by: products of bf16 values are exact in fp32, so a dot product over the
                      dim padded to 16 and the sum over the query's n_q vectors differ from float64 by at most
                      (dpad16 + n_q) 2^-24 times the magnitudes; the factor 2 covers the unknown order of the additions.
Documents are (tok [n_tok, d], off [n_docs + 1]); queries (qtok, qoff) the same way.  A document without vectors has T = S = NaN.
"""

import numpy as np

POISON = 0xFFFFFFFF   # what the test hook fills the screen distances with before the launch
NAN_BITS = 0x7FC00000  # what the kernels write for a document without vectors


def bf16_rn(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 -> fp32, round to nearest even on the bit pattern (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _seg_max(P: np.ndarray, s: np.ndarray, e: np.ndarray) -> np.ndarray:
    """max of P[:, s[i]:e[i]] per i (every segment non-empty, segments ascending and disjoint) -> [rows, len(s)]"""
    if len(s) == 0:
        return np.empty((P.shape[0], 0))
    Pp = np.concatenate([P, np.full((P.shape[0], 1), -np.inf)], axis=1)  # (a segment may end at the last column)
    idx = np.empty(2 * len(s), dtype=np.int64)
    idx[0::2], idx[1::2] = s, e
    return np.maximum.reduceat(Pp, idx, axis=1)[:, 0::2]


def col_max(q: np.ndarray, tok: np.ndarray, off: np.ndarray, variant: str = "own", chunk: int = 1 << 16) -> np.ndarray:
    """M[i, doc] = max_j <q_i, d_j> in float64 (NaN where the variant does not exist for the document).  Variants of a document's
    token set: "own"; "drop_first" / "drop_last" (documents of >= 2 tokens); "add_prev" / "add_next": with the last token of the
    nearest document with tokens in front / the first token of the nearest one behind -- what lies next to it in memory."""
    off = np.asarray(off, np.int64)
    lens = np.diff(off)
    n_docs = len(lens)
    q64, t64 = q.astype(np.float64), tok.astype(np.float64)
    out = np.full((q.shape[0], n_docs), np.nan)
    has = lens > 0
    if variant in ("drop_first", "drop_last"):
        has = lens >= 2
    docs = np.nonzero(has)[0]
    s, e = off[:-1][docs].copy(), off[1:][docs].copy()
    if variant == "drop_first":
        s += 1
    if variant == "drop_last":
        e -= 1
    # (documents in chunks of about `chunk` tokens: the product matrix stays small)
    d0 = 0
    while d0 < len(docs):
        d1 = d0 + 1
        while d1 < len(docs) and e[d1] - s[d0] <= chunk:
            d1 += 1
        lo, hi = off[docs[d0]], off[docs[d1 - 1] + 1]
        P = q64 @ t64[lo:hi].T
        out[:, docs[d0:d1]] = _seg_max(P, s[d0:d1] - lo, e[d0:d1] - lo)
        d0 = d1
    if variant in ("add_prev", "add_next"):
        extra = off[:-1] - 1 if variant == "add_prev" else off[1:]
        ok = (lens > 0) & (extra >= 0) & (extra < tok.shape[0])
        dd = np.nonzero(ok)[0]
        X = np.full((q.shape[0], n_docs), np.nan)
        for a in range(0, len(dd), 4096):
            sl = dd[a:a + 4096]
            X[:, sl] = q64 @ t64[extra[sl]].T
        out = np.where(ok[None, :], np.maximum(out, X), np.nan)
    return out


def sum_queries(M: np.ndarray, qoff) -> np.ndarray:
    """-sum of the rows qoff[b] .. qoff[b + 1] of M per query b (a query without vectors: NaN)"""
    qoff = np.asarray(qoff, np.int64)
    out = np.full((len(qoff) - 1, M.shape[1]), np.nan)
    for b in range(len(qoff) - 1):
        if qoff[b + 1] > qoff[b]:
            out[b] = -M[qoff[b]:qoff[b + 1]].sum(axis=0)
    return out


def T_ref(qtok, qoff, tok, off, variant: str = "own") -> np.ndarray:
    """[B, n_docs] float64; a query without vectors is a row of NaN"""
    return sum_queries(col_max(bf16_rn(qtok), bf16_rn(tok), off, variant), qoff)


def S_ref(qtok, qoff, tok, off) -> np.ndarray:
    return sum_queries(col_max(np.asarray(qtok, np.float32), np.asarray(tok, np.float32), off), qoff)


def _norms(x: np.ndarray) -> np.ndarray:
    return np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))


def E_ref(qtok, qoff, tok, d: int) -> np.ndarray:
    """[B] the bound of csrc/mi355dr_maxsim.hip over the store `tok` (every token of every document that has vectors NOW).
    Measured form: per token pair |q16.d16 - q.d| <= |r_q||d16| + |q||r_d| with r = x - bf16(x), plus the fp32 accumulation of both
    dot products and of the sum over the query, (3 d + 2 n_q) 2^-24 |q||d|; capped by the a-priori form
    (2^-7 + 2^-15 + 3 d 2^-24 + 2 n_q 2^-24) Dmax sum_i |q_i|."""
    tok = np.asarray(tok, np.float32)
    t16 = bf16_rn(tok)
    Dmax, D16max = _norms(tok).max(), _norms(t16).max()
    Rmax = _norms(tok.astype(np.float64) - t16.astype(np.float64)).max()
    qtok = np.asarray(qtok, np.float32)
    qn = _norms(qtok)
    qr = _norms(qtok.astype(np.float64) - bf16_rn(qtok).astype(np.float64))
    qoff = np.asarray(qoff, np.int64)
    out = np.zeros(len(qoff) - 1)
    for b in range(len(qoff) - 1):
        sl = slice(qoff[b], qoff[b + 1])
        nq = qoff[b + 1] - qoff[b]
        norm_sum, res_sum = qn[sl].sum(), qr[sl].sum()
        measured = res_sum * D16max + norm_sum * Rmax + (3.0 * d + 2.0 * nq) * 2.0 ** -24 * Dmax * norm_sum
        apriori = (2.0 ** -7 + 2.0 ** -15 + 3.0 * d * 2.0 ** -24 + 2.0 * nq * 2.0 ** -24) * Dmax * norm_sum
        out[b] = min(measured, apriori)
    return out


def tol_ref(qtok, qoff, tok, off, d: int) -> np.ndarray:
    """[B, n_docs]: 2 (dpad16 + n_q) 2^-24 max_j |bf16(d_j)| sum_i |bf16(q_i)|"""
    off = np.asarray(off, np.int64)
    qoff = np.asarray(qoff, np.int64)
    tn = _norms(bf16_rn(tok))
    lens = np.diff(off)
    dmax = np.zeros(len(lens))
    docs = np.nonzero(lens > 0)[0]
    if len(docs):
        dmax[docs] = _seg_max(tn[None, :], off[:-1][docs], off[1:][docs])[0]
    qn = _norms(bf16_rn(qtok))
    dpad16 = (d + 15) // 16 * 16
    out = np.zeros((len(qoff) - 1, len(lens)))
    for b in range(len(qoff) - 1):
        nq = qoff[b + 1] - qoff[b]
        out[b] = 2.0 * (dpad16 + nq) * 2.0 ** -24 * dmax * qn[qoff[b]:qoff[b + 1]].sum()
    return out
