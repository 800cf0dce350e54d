"""CPU reference of the sparse store (include/mi355dr.h "sparse store"), restated in numpy float64 for the tests.

One elementwise numpy operation per operation of the contract, so every intermediate is rounded once, as an IEEE double:
    avgdl  = total_len / N                          (documents without tokens are no documents)
    norm_i = k1 * ((1.0 - b) + b * (L_i / avgdl))
    for t in the query's terms, ASCENDING:          score[docs of t] = score[docs of t] + w_t * ((tf * (k1 + 1.0)) / (tf + norm))
    distance = -score; a document matches iff it holds a query term
    list = the first k matches under (distance asc, NaN last, id asc), NaN / -1 behind them
The idf of the BM25 layer is math.log -- the libm log the library calls on the host.
"""

import math

import numpy as np

TERM_LIMIT = 1 << 20


class SparseCorpus:
    """Documents as token lists -> per term: (ascending doc ids, tf as float64); lengths; df."""

    def __init__(self, docs=()):
        self.docs = []
        self.add(docs)

    def add(self, docs):
        self.docs.extend([int(t) for t in d] for d in docs)
        self.lengths = np.array([len(d) for d in self.docs], dtype=np.float64)
        self.n_live = int((self.lengths > 0).sum())
        self.total_len = int(self.lengths.sum())
        post = {}
        for i, d in enumerate(self.docs):
            terms, counts = np.unique(np.asarray(d, dtype=np.int64), return_counts=True)
            for t, c in zip(terms.tolist(), counts.tolist()):
                post.setdefault(t, ([], []))
                post[t][0].append(i)
                post[t][1].append(c)
        self.post = {t: (np.asarray(ids, dtype=np.int64), np.asarray(tf, dtype=np.float64)) for t, (ids, tf) in post.items()}

    @classmethod
    def from_flat(cls, terms, offsets):
        """The same from (terms, offsets [n + 1]) without a Python loop per document (tools/time_bm25.py: a million
        documents); `docs` is not kept."""
        self = cls()
        terms, offsets = np.asarray(terms, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        self.docs = None
        self.lengths = np.diff(offsets).astype(np.float64)
        self.n_live = int((self.lengths > 0).sum())
        self.total_len = int(self.lengths.sum())
        key, tf = np.unique(terms * n + np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets)), return_counts=True)
        t_of, d_of = key // n, key % n            # term-major, documents ascending inside a term
        cut = np.flatnonzero(np.diff(t_of)) + 1
        starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [len(key)]])
        self.post = {int(t_of[a]): (d_of[a:b], tf[a:b].astype(np.float64)) for a, b in zip(starts.tolist(), ends.tolist()) if b > a}
        return self

    def __len__(self):
        return len(self.lengths)

    def df(self, t):
        return len(self.post[t][0]) if t in self.post else 0

    @property
    def n_postings(self):
        return sum(len(ids) for ids, _ in self.post.values())

    @property
    def vocab(self):
        return max(self.post) + 1 if self.post else 0


def norms(corpus, k1, b):
    k1, b = np.float64(k1), np.float64(b)
    avgdl = np.float64(corpus.total_len) / np.float64(corpus.n_live)
    r = corpus.lengths / avgdl
    x = b * r
    y = (np.float64(1.0) - b) + x
    return k1 * y


def sort_matches(score, matched, k, row_offset=0):
    """(distance asc, NaN last, id asc): a stable argsort of the matches' distances, which are in id order"""
    ids = np.flatnonzero(matched)
    dist = -score[ids]
    order = np.argsort(dist, kind="stable")[:k]
    out_d = np.full(k, np.nan, dtype=np.float64)
    out_r = np.full(k, -1, dtype=np.int64)
    out_d[:len(order)] = dist[order]
    out_r[:len(order)] = ids[order] + row_offset
    return out_d, out_r


def search_weighted(corpus, queries, k, k1=1.2, b=0.75, row_offset=0):
    """queries: a list of (terms, weights) with distinct terms.  -> (dist [B, k] float64, ids [B, k] int64)"""
    B = len(queries)
    dist = np.full((B, k), np.nan, dtype=np.float64)
    rows = np.full((B, k), -1, dtype=np.int64)
    if corpus.n_live == 0:
        return dist, rows
    norm = norms(corpus, k1, b)
    k1p1 = np.float64(k1) + np.float64(1.0)
    for j, (terms, weights) in enumerate(queries):
        score = np.zeros(len(corpus), dtype=np.float64)
        matched = np.zeros(len(corpus), dtype=bool)
        for t, w in sorted(zip([int(t) for t in terms], [float(w) for w in weights])):
            if t not in corpus.post:
                continue
            ids, tf = corpus.post[t]
            with np.errstate(all="ignore"):
                num = tf * k1p1
                den = tf + norm[ids]
                frac = num / den
                score[ids] = score[ids] + np.float64(w) * frac
            matched[ids] = True
        dist[j], rows[j] = sort_matches(score, matched, k, row_offset)
    return dist, rows


def bm25_weights(corpus, tokens):
    """raw query tokens -> (terms ascending, each once, df > 0; idf weights by math.log)"""
    terms = [t for t in sorted(set(int(t) for t in tokens)) if 0 <= t < TERM_LIMIT and corpus.df(t) > 0]
    N = corpus.n_live
    return terms, [math.log(1.0 + ((float(N - corpus.df(t)) + 0.5) / (float(corpus.df(t)) + 0.5))) for t in terms]


def search_bm25(corpus, token_lists, k, k1=1.2, b=0.75, row_offset=0):
    return search_weighted(corpus, [bm25_weights(corpus, q) for q in token_lists], k, k1, b, row_offset)


def score_scalar(corpus, terms, weights, k1, b):
    """the contract as a scalar Python loop (Python floats are IEEE doubles): {doc id: distance} of the matches"""
    avgdl = float(corpus.total_len) / float(corpus.n_live)
    out = {}
    for i, d in enumerate(corpus.docs):
        if not d:
            continue
        norm = k1 * ((1.0 - b) + b * (float(len(d)) / avgdl))
        score, hit = 0.0, False
        for t, w in sorted(zip(terms, weights)):
            tf = d.count(t)
            if tf > 0:
                frac = (float(tf) * (k1 + 1.0)) / (float(tf) + norm)
                score = score + (w * frac)
                hit = True
        if hit:
            out[i] = -score
    return out


_ref_weighted, _ref_bm25 = search_weighted, search_bm25  # (sparse_methods defines methods of the same names)


def sparse_methods(cls):
    """Class decorator: the sparse methods of Mi355Index (add_sparse, size_sparse, sparse_df, search_sparse, search_bm25),
    answered by this reference -- the host stand-in of the pipeline tests."""

    def _corpus(self):
        if getattr(self, "_sparse", None) is None:
            self._sparse = SparseCorpus()
        return self._sparse

    def add_sparse(self, token_lists, offsets=None):
        if offsets is not None:
            token_lists = [list(token_lists[offsets[i]:offsets[i + 1]]) for i in range(len(offsets) - 1)]
        _corpus(self).add(token_lists)

    def size_sparse(self):
        return len(_corpus(self))

    def sparse_df(self, terms):
        return np.array([_corpus(self).df(int(t)) for t in terms], dtype=np.int64)

    def search_sparse(self, terms, weights, offsets, k, k1=1.2, b=0.75, device_out=False):
        qs = [(list(terms[offsets[i]:offsets[i + 1]]), list(weights[offsets[i]:offsets[i + 1]])) for i in range(len(offsets) - 1)]
        return _ref_weighted(_corpus(self), qs, k, k1, b, getattr(self, "row_offset", 0))

    def search_bm25(self, token_lists, k, k1=1.2, b=0.75, device_out=False, offsets=None):
        return _ref_bm25(_corpus(self), token_lists, k, k1, b, getattr(self, "row_offset", 0))

    for f in (add_sparse, size_sparse, sparse_df, search_sparse, search_bm25):
        setattr(cls, f.__name__, f)
    if not hasattr(cls, "close"):
        cls.close = lambda self: None
    return cls


@sparse_methods
class SparseRefIndex:
    """A host stand-in with nothing but the sparse store."""

    def __init__(self, dim=8, metric="cosine", device=0):
        self.dim, self.metric, self.device, self.row_offset = dim, metric, device, 0
