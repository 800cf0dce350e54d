"""Reference of "MaxSim explained" (include/mi355dr.h: mi355dr_multivec_token_counts / _maxsim_align / _maxsim_map): numpy plus one
`cpu_ref.dot` per (query vector, token) pair.  Keep corpora tiny: every dot is a ctypes call.

The rule, restated:
  * every dot is oracle.c's orc_dot, the k-ascending fp32 fmaf chain from 0.0f;
  * the maximum of a query vector over a document is fmaxf from -inf over the tokens in order: a NaN dot is ignored;
  * the token is the LOWEST j with dot_j == maximum (float equality); no such j (every dot NaN): value -inf, token -1;
  * clamp0 replaces the value by max(0, value); the token stays that of the unclamped maximum;
  * a candidate whose id is outside the store (negative and -1 padding included) or whose document has no vectors: value NaN,
    token -1, distance NaN;
  * distance = 0.0f, then acc = acc + (-value) per query vector in order, in fp32; a query without vectors: NaN;
  * a map is the plain matrix of dots [nq, T]; a skipped document or a query without vectors gives an empty map.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import cpu_ref

F32 = np.float32


class Alignment(NamedTuple):
    values: np.ndarray   # [V, m] float32
    tokens: np.ndarray   # [V, m] int32
    dist: np.ndarray     # [B, m] float32


def dots(q: np.ndarray, doc: np.ndarray) -> np.ndarray:
    """[nq, T] float32, every element one orc_dot"""
    out = np.empty((q.shape[0], doc.shape[0]), dtype=F32)
    for i in range(q.shape[0]):
        for j in range(doc.shape[0]):
            out[i, j] = cpu_ref.dot(q[i], doc[j])
    return out


def row_max(row: np.ndarray) -> tuple[np.float32, int]:
    """(maximum, lowest index that holds it) of one row of dots: fmaxf from -inf, NaN ignored; (-inf, -1) when all are NaN"""
    m = F32(-np.inf)
    for v in row:
        if not np.isnan(v) and v > m:
            m = F32(v)
    hit = np.nonzero(row == m)[0]
    return m, (int(hit[0]) if hit.size else -1)


def fold(values) -> np.float32:
    """the distance chain over one candidate's (already clamped) values, in vector order"""
    acc = F32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in values:
            acc = F32(acc + F32(-v))
    return acc


class RefStore:
    """The multi-vector store on the host with the three entry points (and maxsim_subset, for the service's stand-in): the
    surface of Mi355Index that ShardedSearcher and the service touch."""

    def __init__(self, dim: int, metric: str = "cosine", device: int = 0):
        self.dim, self.docs, self.row_offset = dim, [], 0

    def set_option(self, key, value):
        if key == "row_offset":
            self.row_offset = int(value)

    def add_multivec(self, vecs, offsets):
        vecs = np.ascontiguousarray(vecs, dtype=F32).reshape(-1, self.dim)
        for a, b in zip(offsets[:-1], offsets[1:]):
            self.docs.append(vecs[int(a):int(b)].copy())

    def set_multivec(self, doc_ids, vecs, offsets):
        vecs = np.ascontiguousarray(vecs, dtype=F32).reshape(-1, self.dim)
        for i, a, b in zip(doc_ids, offsets[:-1], offsets[1:]):
            self.docs[int(i)] = vecs[int(a):int(b)].copy()

    def n_docs(self):
        return len(self.docs)

    def close(self):
        pass

    def _doc(self, gid):
        i = int(gid) - self.row_offset
        return self.docs[i] if 0 <= i < len(self.docs) else None

    def multivec_token_counts(self, doc_ids) -> np.ndarray:
        ids = np.asarray(doc_ids, dtype=np.int64).reshape(-1)
        return np.array([-1 if self._doc(g) is None else self._doc(g).shape[0] for g in ids], dtype=np.int32)

    def maxsim_align(self, qtok, q_offsets, doc_ids, clamp0=False, want_dist=True) -> Alignment:
        q = np.ascontiguousarray(qtok, dtype=F32).reshape(-1, self.dim)
        qo = np.asarray(q_offsets, dtype=np.int64)
        ids = np.asarray(doc_ids, dtype=np.int64)
        B, m = ids.shape
        V = int(qo[B] - qo[0])
        val = np.full((V, m), np.nan, dtype=F32)
        tok = np.full((V, m), -1, dtype=np.int32)
        dist = np.full((B, m), np.nan, dtype=F32)
        for b in range(B):
            g0, g1 = int(qo[b] - qo[0]), int(qo[b + 1] - qo[0])
            for p in range(m):
                doc = self._doc(ids[b, p])
                if doc is None or doc.shape[0] == 0 or g1 == g0:
                    continue
                dd = dots(q[int(qo[b]):int(qo[b + 1])], doc)
                for i in range(g1 - g0):
                    v, t = row_max(dd[i])
                    val[g0 + i, p] = max(v, F32(0.0)) if clamp0 else v
                    tok[g0 + i, p] = t
                dist[b, p] = fold(val[g0:g1, p])
        return Alignment(val, tok, dist if want_dist else None)

    def maxsim_map(self, qtok, q_offsets, pair_query, pair_doc) -> list[np.ndarray]:
        q = np.ascontiguousarray(qtok, dtype=F32).reshape(-1, self.dim)
        qo = np.asarray(q_offsets, dtype=np.int64)
        out = []
        for b, g in zip(np.asarray(pair_query).reshape(-1), np.asarray(pair_doc).reshape(-1)):
            doc = self._doc(g)
            qb = q[int(qo[b]):int(qo[b + 1])]
            out.append(dots(qb, doc if doc is not None else np.zeros((0, self.dim), F32)))
        return out

    def maxsim_subset(self, qtok, q_offsets, doc_ids, clamp0=False) -> np.ndarray:
        return self.maxsim_align(qtok, q_offsets, doc_ids, clamp0=clamp0).dist


def same_bits(a, b):
    """float32 arrays equal bit for bit where they are numbers, NaN at the same places"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    assert np.array_equal(a[ok].view(np.uint32), b[ok].view(np.uint32))


def same_alignment(got, want):
    same_bits(got.values, want.values)
    assert np.array_equal(np.asarray(got.tokens), np.asarray(want.tokens))
    assert (got.dist is None) == (want.dist is None)
    if want.dist is not None:
        same_bits(got.dist, want.dist)
