"""The source cap of include/mi355dr.h ("source-capped lists and search") as a plain loop, the inputs the GPU tests share, and
the comparison they use.  No GPU, no library: numpy only."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

INT64_MAX = np.iinfo(np.int64).max
NAN_BITS = np.uint64(0x7FF8000000000000)
TRUNCATED = 1


class Collapsed(NamedTuple):
    vals: np.ndarray      # float64 [B, k_out]
    ids: np.ndarray       # int64 [B, k_out]
    keys: np.ndarray      # int64 [B, k_out]
    pos: np.ndarray       # int32 [B, k_out]
    count: np.ndarray     # int32 [B]: kept entries of the whole list
    entries: np.ndarray   # int32 [B]


def key_of(keys, entry_id: int):
    """(has a key, the key) of an entry with id `entry_id` >= 0."""
    if keys is None or entry_id >= len(keys) or int(keys[entry_id]) < 0:
        return False, -1
    return True, int(keys[entry_id])


def collapse(vals, ids, keys, cap: int, k_out: int) -> Collapsed:
    """The walk, list by list, entry by entry."""
    vals = np.asarray(vals, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64)
    B, w = ids.shape
    out_v = np.full((B, k_out), np.nan, dtype=np.float64)
    out_v.view(np.uint64)[:] = NAN_BITS
    out_i = np.full((B, k_out), -1, dtype=np.int64)
    out_k = np.full((B, k_out), -1, dtype=np.int64)
    out_p = np.full((B, k_out), -1, dtype=np.int32)
    count = np.zeros(B, dtype=np.int32)
    entries = np.zeros(B, dtype=np.int32)
    vbits, obits = vals.view(np.uint64), out_v.view(np.uint64)
    for b in range(B):
        seen: dict[int, int] = {}
        kept = 0
        for s in range(w):
            e = int(ids[b, s])
            if e < 0:
                continue
            entries[b] += 1
            has, key = key_of(keys, e)
            if has:
                n = seen.get(key, 0)
                seen[key] = n + 1
                if n >= cap:
                    continue
            if kept < k_out:
                obits[b, kept] = vbits[b, s]
                out_i[b, kept] = e
                out_k[b, kept] = key
                out_p[b, kept] = s
            kept += 1
        count[b] = kept
    return Collapsed(out_v, out_i, out_k, out_p, count, entries)


def collapse_by_rank(vals, ids, keys, cap: int, k_out: int) -> Collapsed:
    """A second formulation, independent of the loop: an entry's rank within its key by ONE stable sort of the list's keyed
    entries; kept = no key or rank < cap; output slots by a cumulative sum."""
    vals = np.asarray(vals, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64)
    B, w = ids.shape
    table = None if keys is None else np.asarray(keys, dtype=np.int64)
    out_v = np.empty((B, k_out), dtype=np.float64)
    out_v.view(np.uint64)[:] = NAN_BITS
    out_i = np.full((B, k_out), -1, dtype=np.int64)
    out_k = np.full((B, k_out), -1, dtype=np.int64)
    out_p = np.full((B, k_out), -1, dtype=np.int32)
    count = np.zeros(B, dtype=np.int32)
    entries = np.zeros(B, dtype=np.int32)
    for b in range(B):
        entry = ids[b] >= 0
        key = np.full(w, -1, dtype=np.int64)
        if table is not None and len(table):
            inside = entry & (ids[b] < len(table))
            key[inside] = table[ids[b][inside]]
        has = entry & (key >= 0)
        rank = np.zeros(w, dtype=np.int64)
        at = np.flatnonzero(has)
        order = at[np.argsort(key[at], kind="stable")]            # keys side by side, list order inside a key
        sk = key[order]
        start = np.r_[True, sk[1:] != sk[:-1]] if len(sk) else np.zeros(0, dtype=bool)
        first = np.maximum.accumulate(np.where(start, np.arange(len(sk)), 0)) if len(sk) else np.zeros(0, dtype=np.int64)
        rank[order] = np.arange(len(sk)) - first
        kept = entry & (~has | (rank < cap))
        slot = np.cumsum(kept) - 1
        take = np.flatnonzero(kept & (slot < k_out))
        out_v.view(np.uint64)[b, slot[take]] = vals.view(np.uint64)[b, take]
        out_i[b, slot[take]] = ids[b, take]
        out_k[b, slot[take]] = np.where(has[take], key[take], -1)
        out_p[b, slot[take]] = take
        count[b] = int(kept.sum())
        entries[b] = int(entry.sum())
    return Collapsed(out_v, out_i, out_k, out_p, count, entries)


def same(got, exp: Collapsed, what: str = "") -> None:
    """Every field the call returned (None: switched off) against the reference: values as BITS."""
    names = ("vals", "ids", "keys", "pos", "count", "entries")
    for name, g, e in zip(names, got, exp):
        if g is None:
            continue
        g = np.asarray(g)
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        if name == "vals":
            g, e = g.view(np.uint64), e.view(np.uint64)
        bad = np.argwhere(g != e)
        assert bad.size == 0, f"{what}: {name} differs at {bad[:5].tolist()}: got {g[tuple(bad[0])]}, expected {e[tuple(bad[0])]}"


def search_result(full_dist, full_rows, keys, cap: int, k: int, max_fetch: int):
    """What search_collapsed returns, from the exact search at max_fetch: (dist, rows, keys, count, state)."""
    c = collapse(full_dist[:, :max_fetch], full_rows[:, :max_fetch], keys, cap, k)
    count = np.minimum(c.count, k).astype(np.int32)
    state = np.where((c.count < k) & (c.entries >= max_fetch), TRUNCATED, 0).astype(np.int32)
    return c.vals, c.ids, c.keys, count, state


def same_search(got, exp, what: str = "") -> None:
    for name, g, e in zip(("dist", "rows", "keys", "count", "state"), got, exp):
        g = np.asarray(g)
        assert g.shape == e.shape and g.dtype == e.dtype, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        if name == "dist":
            g, e = g.view(np.uint64), e.view(np.uint64)
        bad = np.argwhere(g != e)
        assert bad.size == 0, f"{what}: {name} differs at {bad[:5].tolist()}: got {g[tuple(bad[0])]}, expected {e[tuple(bad[0])]}"


# ---- the hand cases: (name, vals [B,w], ids [B,w], keys or None, cap, k_out, expected ids of line 0, expected count of line 0)
def hand_cases():
    f = lambda *v: np.array([v], dtype=np.float64)  # noqa: E731
    i = lambda *v: np.array([v], dtype=np.int64)    # noqa: E731
    keys = np.array([5, 5, 5, 9, -1, INT64_MAX, INT64_MAX, -7, 1 << 40, 1 << 40], dtype=np.int64)
    return [
        ("cap 1 keeps the first of a key", f(.1, .2, .3, .4), i(0, 1, 2, 3), keys, 1, 4, [0, 3, -1, -1], 2),
        ("cap 2 keeps two", f(.1, .2, .3, .4), i(0, 1, 2, 3), keys, 2, 4, [0, 1, 3, -1], 3),
        ("no key is never capped", f(.1, .2, .3, .4), i(4, 7, 4, 7), keys, 1, 4, [4, 7, 4, 7], 4),
        ("INT64_MAX is a key", f(.1, .2, .3), i(5, 6, 4), keys, 1, 3, [5, 4, -1], 2),
        ("keys above 2^32", f(.1, .2, .3), i(8, 9, 3), keys, 1, 3, [8, 3, -1], 2),
        ("an id beyond the table has no key", f(.1, .2, .3), i(10, 10, 11), keys, 1, 3, [10, 10, 11], 3),
        ("an id listed twice is two entries", f(.1, .2, .3), i(0, 0, 0), keys, 2, 3, [0, 0, -1], 2),
        ("a hole in the middle is no entry", f(.1, .2, .3, .4), i(0, -1, 3, 1), keys, 1, 4, [0, 3, -1, -1], 2),
        ("a null table keeps everything", f(.1, .2, .3), i(0, 1, 2), None, 1, 3, [0, 1, 2], 3),
        ("count may exceed k_out", f(.1, .2, .3, .4), i(3, 4, 7, 8), keys, 1, 2, [3, 4], 4),
        ("an empty list", f(.1, .2), i(-1, -1), keys, 1, 2, [-1, -1], 0),
    ]


# ---- the inputs of the GPU list tests: (name, vals, ids, keys, cap)
def _vals(rng, B, w):
    v = np.sort(rng.standard_normal((B, w)), axis=1)
    return np.ascontiguousarray(v, dtype=np.float64)


def all_inputs():
    """Every (name, vals [B,w], ids [B,w], keys | None, cap) the list forms are held to: the widths 1 .. 4096 (1025 pads to
    2048), the caps, the key patterns, the key values and the id patterns of the contract.  Seeded: the same on every call."""
    rng = np.random.default_rng(11)
    out = []
    widths = (1, 63, 64, 65, 257, 1024, 1025, 4096)
    for w in widths:
        B = 3
        ids = np.stack([rng.permutation(w + 50)[:w] for _ in range(B)]).astype(np.int64)
        n_ids = w + 50
        patterns = {
            "one key": np.full(n_ids, 3, dtype=np.int64),
            "distinct": np.arange(n_ids, dtype=np.int64) + (1 << 33),
        }
        caps = sorted({1, 2, 3, 64, w})
        for pname, table in patterns.items():
            for cap in caps:
                out.append((f"w={w} {pname} cap={cap}", _vals(rng, B, w), ids, table, cap))
        # keys by POSITION in the list: pos % 3 and pos // 5 (the table is built through the ids of line 0 and used for it alone)
        for pname, fn in (("pos%3", lambda p: p % 3), ("pos//5", lambda p: p // 5)):
            table = np.full(n_ids, -1, dtype=np.int64)
            table[ids[0]] = fn(np.arange(w))
            for cap in caps:
                out.append((f"w={w} {pname} cap={cap}", _vals(rng, 1, w), ids[:1], table, cap))
        # a run of exactly cap entries and one of cap + 1, separated by other keys
        for cap in caps:
            if 2 * cap + 2 > w:
                continue
            table = np.arange(n_ids, dtype=np.int64) + 100
            table[ids[0][:cap]] = 7
            table[ids[0][cap + 1:2 * cap + 2]] = 8
            out.append((f"w={w} runs of cap and cap+1, cap={cap}", _vals(rng, 1, w), ids[:1], table, cap))
    # key values and id patterns at a width that crosses one wave and one at the top
    for w in (65, 1025):
        n_ids = w + 20
        table = rng.integers(0, 6, size=n_ids).astype(np.int64)
        table[::7] = INT64_MAX
        table[1::7] = (1 << 40) + 5
        table[2::7] = -1
        table[3::7] = -7
        base = rng.integers(0, n_ids + 30, size=(3, w)).astype(np.int64)     # repeats, and ids at or beyond keys_len
        base[0, w // 2] = -1                                                  # a hole in the middle
        base[1, w - 9:] = -1                                                  # tails of different lengths
        base[2, w - 40:] = -1
        base[2, 3] = base[2, 0]                                               # an id listed twice, on purpose
        v = _vals(rng, 3, w)
        v[0, 5] = np.nan                                                      # NaN with an id: an entry
        v[0, 6], v[0, 7] = 0.0, -0.0
        v[1, 0], v[1, 1] = -np.inf, np.inf
        v.view(np.uint64)[2, 1] = np.uint64(0x7FF80000DEADBEEF)               # a NaN payload
        for cap in (1, 2):
            out.append((f"w={w} mixed keys and ids cap={cap}", v, base, table, cap))
        out.append((f"w={w} null table", v, base, None, 1))
        big = base.copy()
        big[big >= 0] += (1 << 31) + 12345                                    # ids above 2^31: beyond any table here
        out.append((f"w={w} ids above 2^31", v, big, table, 1))
        out.append((f"w={w} all -1", v, np.full((3, w), -1, dtype=np.int64), table, 1))
    return out


# ---- the corpora of the search tests (default_rng(7), d = 64, 5 queries); each returns (C float32, Q float32, keys int64)
def _queries_and_rows(n):
    rng = np.random.default_rng(7)
    Q = rng.standard_normal((5, 64)).astype(np.float32)
    C = rng.standard_normal((n, 64)).astype(np.float32)
    return rng, Q, C


def corpus_a():
    """4096 Gaussian rows, sources of 4 consecutive rows; rows 1000 .. 1299 are near-copies of query 0 and share ONE source:
    query 0 finds its 10th kept entry some 300 entries deep, the other queries at depth 10 or 11."""
    rng, Q, C = _queries_and_rows(4096)
    C[1000:1300] = Q[0] + 0.05 * rng.standard_normal((300, 64)).astype(np.float32)
    keys = (np.arange(4096) // 4).astype(np.int64)
    keys[1000:1300] = 250
    return C, Q, keys


def corpus_b():
    """2048 rows; rows 100 .. 1199 are near query 1 and share one source, every other row is its own: at max_fetch = 1024 query
    1's ranking is cut inside the heavy source."""
    rng, Q, C = _queries_and_rows(2048)
    C[100:1200] = Q[1] + 0.05 * rng.standard_normal((1100, 64)).astype(np.float32)
    keys = np.arange(2048, dtype=np.int64) + (1 << 34)
    keys[100:1200] = 5
    return C, Q, keys


def corpus_c():
    """50 rows, three of them zero: under cosine their distances are NaN, they come last in the ranking and are still entries."""
    rng, Q, C = _queries_and_rows(50)
    C[[7, 20, 41]] = 0.0
    return C, Q, (np.arange(50) // 4).astype(np.int64)


def depth_of_kth(full_rows, keys, cap: int, k: int):
    """Per query: the 1-based depth of the k-th kept entry in the ranking `full_rows` [B, m] (0: fewer than k are kept)."""
    c = collapse(np.zeros(full_rows.shape), full_rows, keys, cap, k)
    return np.where(c.count >= k, c.pos[:, k - 1] + 1, 0)


def expected_researched(full_rows, keys, cap: int, k: int, fetch_k: int, max_fetch: int) -> int:
    """(query, round) re-searches of the schedule in include/mi355dr.h, replayed over the ranking at max_fetch."""
    total = 0
    for b in range(full_rows.shape[0]):
        f = fetch_k
        while True:
            c = collapse(np.zeros((1, f)), full_rows[b:b + 1, :f], keys, cap, k)
            if c.count[0] >= k or c.entries[0] < f or f >= max_fetch:
                break
            f = min(2 * f, max_fetch)
            total += 1
    return total
