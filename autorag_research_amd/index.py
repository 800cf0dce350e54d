"""Mi355Index -- Python handle over one libmi355dr index (one GPU, one corpus shard).

Replaces what BaseVectorRepository asked PostgreSQL to do (reference
autorag_research/orm/repository/base.py:378-426 `<=>`, :487-571 `@#`): it owns the rows in HBM and
answers exact top-k.  Rows are dense indices in insertion order; id mapping lives in store.py.
"""

from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _native
from ._native import NativeError, check, f32c, ptr

METRICS = {"cosine": 0, "ip": 1}
PATHS = {"auto": 0, "screen": 1, "scan": 2}
SCREEN_DTYPES = {"auto": 0, "bf16": 1, "i8": 2}
FUSE_METHODS = {"rrf": 0, "mm": 1, "tmm": 2, "z": 3, "dbsf": 4}      # MI355DR_FUSE_RRF / _CC_*
FUSE_MODES = {"one_minus": 0, "negate": 1, "as_is": 2}               # MI355DR_FUSE_ONE_MINUS / _NEGATE / _AS_IS


COLLAPSE_TRUNCATED = 1   # MI355DR_COLLAPSE_TRUNCATED: fewer than k kept although the ranking was cut at max_fetch
# search_collapsed's first round is searched at COLLAPSE_FETCH_MULT * k unless the caller says otherwise.  The rule
# (profiles/collapse_timing.txt): the multiple of k that is cheapest where every source holds 8
# near-copies AND costs a corpus whose cap almost never bites no more than the table's box-to-box noise over fetch_k = k.
# Measured at 1 M x 768, 1024 queries, k = 10: 2 k costs the Gaussian corpus 1.13 ms against 1.03 (+9 %) where two boxes differ
# by under 4 %, so no multiple above 1 qualifies.  A corpus of near-copies is served best by a caller's fetch_k of about 4 k
# (6.5 ms against 12.4).
COLLAPSE_FETCH_MULT = 1


class CollapsedLists(NamedTuple):
    """`Mi355Index.collapse_lists`: the kept entries of each list; a field the call switched off is None."""

    vals: np.ndarray
    ids: np.ndarray
    keys: np.ndarray | None
    pos: np.ndarray | None
    count: np.ndarray | None
    entries: np.ndarray | None


class CollapsedSearch(NamedTuple):
    """`Mi355Index.search_collapsed*`: at most `cap` rows per source."""

    dist: np.ndarray
    rows: np.ndarray
    keys: np.ndarray
    count: np.ndarray
    state: np.ndarray


class MaxSimAlignment(NamedTuple):
    """`Mi355Index.maxsim_align`: per query vector (V in all, in query order) and candidate position the matched token."""

    values: np.ndarray        # [V, m] float32: max_j <q_i, d_j> (clamp0: max(0, .)); NaN = candidate skipped
    tokens: np.ndarray        # [V, m] int32: the lowest token index that reaches the unclamped maximum; -1 = none
    dist: np.ndarray | None   # [B, m] float32: the bits of `maxsim_subset`; None when not asked for


class DeviceKeys:
    """A key table on an index's device (`Mi355Index.upload_keys`): int64 [length] at `ptr`, 0 / 0 for an empty table."""

    def __init__(self, index: "Mi355Index", keys):
        t = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        self._index = index
        self.length = int(t.shape[0])
        self.ptr = 0
        if self.length:
            self.ptr = index.dev_alloc(t.nbytes)
            try:
                index.dev_upload(self.ptr, t)
            except Exception:
                self.close()
                raise

    @classmethod
    def borrowed(cls, ptr: int, length: int) -> "DeviceKeys":
        """A table that lives in a device buffer of the caller's (int64 [length] at `ptr`): close() leaves it alone."""
        self = cls.__new__(cls)
        self._index, self.ptr, self.length = None, int(ptr), int(length)
        return self

    def close(self) -> None:
        if self.ptr:
            p, self.ptr = self.ptr, 0
            if self._index is not None:
                self._index.dev_free(p)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False


def _stream_arg(stream) -> ctypes.c_void_p:
    """A HIP stream handle (int) as the C ABI's `void* stream`; None / 0 = the index's own stream."""
    return ctypes.c_void_p(int(stream) if stream else None)


class Mi355Index:
    def __init__(self, dim: int, metric: str = "cosine", device: int = 0):
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {sorted(METRICS)}")
        self._lib = _native.load()
        self._h = ctypes.c_void_p()
        rc = self._lib.mi355dr_create(ctypes.byref(self._h), int(device), int(dim), METRICS[metric])
        if rc != 0:
            msg = self._lib.mi355dr_last_error(None)
            raise NativeError(rc, msg.decode() if msg else "")
        self.dim = int(dim)
        self.metric = metric
        self.device = int(device)
        self._is_view = False

    # ---- lifetime ----
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.mi355dr_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # noqa: D105
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False

    # ---- corpus ----
    def __len__(self) -> int:
        return int(self._lib.mi355dr_size(self._h))

    def reserve(self, n_rows: int) -> None:
        check(self._h, self._lib.mi355dr_reserve(self._h, int(n_rows)))

    def add(self, rows) -> None:
        rows = f32c(rows)
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}], got {rows.shape}")
        check(self._h, self._lib.mi355dr_add_rows(self._h, ptr(rows, ctypes.c_float), rows.shape[0]))

    def add_device(self, dev_ptr: int, n: int) -> None:
        """Append n rows already resident on this device (fp32, row-major, contiguous)."""
        check(self._h, self._lib.mi355dr_add_rows_device(self._h, ctypes.c_void_p(int(dev_ptr)), int(n)))

    # ---- update / remove in place (row ids are stable; include/mi355dr.h "update / remove in place") ----
    @staticmethod
    def _row_ids(row_ids) -> np.ndarray:
        ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        if ids.ndim != 1:
            raise ValueError("row_ids must be one-dimensional")
        return ids

    def update_rows(self, row_ids, rows) -> None:
        """Row row_ids[j] takes rows[j]: later searches see the index an `add` of the new vectors would have built.
        Updating a removed row revives it.  Ids out of range or repeated: NativeError (MI355DR_E_INVALID), nothing changes."""
        ids = self._row_ids(row_ids)
        rows = f32c(rows)
        if rows.ndim != 2 or rows.shape != (ids.shape[0], self.dim):
            raise ValueError(f"rows must be [{ids.shape[0]}, {self.dim}], got {rows.shape}")
        check(self._h, self._lib.mi355dr_update_rows(self._h, ptr(ids, ctypes.c_int64), ptr(rows, ctypes.c_float), ids.shape[0]))

    def update_rows_device(self, row_ids, dev_ptr: int) -> None:
        """The same with the new rows ([len(row_ids), dim] fp32, contiguous) already on this device; ids stay on the host."""
        ids = self._row_ids(row_ids)
        check(self._h, self._lib.mi355dr_update_rows_device(self._h, ptr(ids, ctypes.c_int64), ctypes.c_void_p(int(dev_ptr)),
                                                            ids.shape[0]))

    def remove_rows(self, row_ids) -> None:
        """The rows are dead: never returned again by any path; their slots (and every other row's id) stay."""
        ids = self._row_ids(row_ids)
        check(self._h, self._lib.mi355dr_remove_rows(self._h, ptr(ids, ctypes.c_int64), ids.shape[0]))

    def compact(self) -> np.ndarray:
        """Drop the removed rows: the live rows keep their order and become rows 0 .. live_rows-1, and the index answers
        like one built fresh by one `add` of them.  Returns new_of_old (int64 [len(self) before the call]): the new id of
        every old row, -1 for a removed one.  Pools for gqr_refine and any row -> key map of the caller follow this map."""
        if not self._h:
            raise ValueError("compact() on a closed index")
        new_of_old = np.empty(len(self), dtype=np.int64)
        check(self._h, self._lib.mi355dr_compact(self._h, ptr(new_of_old, ctypes.c_int64)))
        return new_of_old

    @property
    def live_rows(self) -> int:
        """len(self) minus the removed rows."""
        return int(self._lib.mi355dr_live_rows(self._h))

    def get_rows(self, row0: int, n: int) -> np.ndarray:
        out = np.empty((n, self.dim), dtype=np.float32)
        check(self._h, self._lib.mi355dr_get_rows(self._h, int(row0), int(n), ptr(out, ctypes.c_float)))
        return out

    # ---- search ----
    def search(self, queries, k: int) -> tuple[np.ndarray, np.ndarray]:
        """Exact top-k.  Returns (distance float64 [B,k], rows int64 [B,k]); pads with NaN / -1.

        distance is pgvector's cosine distance (or negative inner product), ordered
        (distance asc, NaN last, row asc) -- the same contract the CPU checker in oracle/ states.
        """
        q = f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [B, {self.dim}], got {q.shape}")
        B = q.shape[0]
        dist = np.empty((B, k), dtype=np.float64)
        rows = np.empty((B, k), dtype=np.int64)
        check(self._h, self._lib.mi355dr_search(self._h, ptr(q, ctypes.c_float), B, int(k),
                                                ptr(dist, ctypes.c_double), ptr(rows, ctypes.c_int64)))
        return dist, rows

    def search_device(self, q_ptr: int, B: int, k: int, out_dist_ptr: int, out_rows_ptr: int,
                      stream: int | None = None) -> None:
        check(self._h, self._lib.mi355dr_search_device(self._h, ctypes.c_void_p(int(q_ptr)), int(B), int(k),
                                                       ctypes.c_void_p(int(out_dist_ptr)),
                                                       ctypes.c_void_p(int(out_rows_ptr)),
                                                       _stream_arg(stream)))

    def search_device_async(self, q_ptr: int, B: int, k: int, out_dist_ptr: int, out_rows_ptr: int,
                            stream: int | None = None) -> int:
        """Enqueue the search and return a ticket without synchronising (mi355dr_search_device_async): the outputs are
        valid after `search_wait(ticket)`; the query and output buffers must stay untouched until then."""
        t = ctypes.c_int64(0)
        check(self._h, self._lib.mi355dr_search_device_async(self._h, ctypes.c_void_p(int(q_ptr)), int(B), int(k),
                                                             ctypes.c_void_p(int(out_dist_ptr)),
                                                             ctypes.c_void_p(int(out_rows_ptr)),
                                                             _stream_arg(stream),
                                                             ctypes.byref(t)))
        return int(t.value)

    def search_wait(self, ticket: int) -> None:
        """Complete every block up to `ticket` (waits, then recomputes the rare queries the screen flagged)."""
        check(self._h, self._lib.mi355dr_search_wait(self._h, int(ticket)))

    # ---- search within a listed subset of rows (include/mi355dr.h "search within a listed subset of rows") ----
    def search_subset(self, queries, k: int, row_ids) -> tuple[np.ndarray, np.ndarray]:
        """Exact top-k among the listed rows only: `search` with `AND id = ANY(row_ids)`.  row_ids: global rows as the
        searches return them, one list for all queries, in any order; ids outside the index (-1 padding included) and
        removed rows are skipped, an id listed twice counts once.  Same distances, order and NaN / -1 tail as `search`."""
        q = f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [B, {self.dim}], got {q.shape}")
        ids = self._row_ids(row_ids)
        B = q.shape[0]
        dist = np.empty((B, k), dtype=np.float64)
        rows = np.empty((B, k), dtype=np.int64)
        check(self._h, self._lib.mi355dr_search_subset(self._h, ptr(q, ctypes.c_float), B, int(k), ptr(ids, ctypes.c_int64),
                                                       ids.shape[0], ptr(dist, ctypes.c_double), ptr(rows, ctypes.c_int64)))
        return dist, rows

    def search_subset_device(self, q_ptr: int, B: int, k: int, row_ids, out_dist_ptr: int, out_rows_ptr: int,
                             stream: int | None = None) -> None:
        """The same with queries and outputs in device memory (the list stays on the host); complete on return."""
        ids = self._row_ids(row_ids)
        check(self._h, self._lib.mi355dr_search_subset_device(
            self._h, ctypes.c_void_p(int(q_ptr)), int(B), int(k), ptr(ids, ctypes.c_int64), ids.shape[0],
            ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)),
            _stream_arg(stream)))

    def score_subset(self, queries, row_ids) -> np.ndarray:
        """Exact distance of each query to its own list of rows: row_ids [B, m] (global) -> float64 [B, m]; NaN for ids
        outside the index, removed rows and undefined distances."""
        q = f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        ids = np.ascontiguousarray(row_ids, dtype=np.int64)
        if ids.ndim == 1:
            ids = ids[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim or ids.ndim != 2 or ids.shape[0] != q.shape[0]:
            raise ValueError(f"queries must be [B, {self.dim}] and row_ids [B, m]")
        out = np.empty(ids.shape, dtype=np.float64)
        check(self._h, self._lib.mi355dr_score_subset(self._h, ptr(q, ctypes.c_float), q.shape[0], ptr(ids, ctypes.c_int64),
                                                      ids.shape[1], ptr(out, ctypes.c_double)))
        return out

    # ---- MMR: a diversity-aware top-k selected on the device (include/mi355dr.h "MMR search") ----
    def _queries_2d(self, queries) -> np.ndarray:
        q = f32c(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries must be [B, {self.dim}], got {q.shape}")
        return q

    def search_mmr(self, queries, k: int, fetch_k: int, lambda_mult: float = 0.5) -> tuple[np.ndarray, np.ndarray]:
        """Maximal Marginal Relevance: the ordinary search at `fetch_k`, then `k` of its results picked greedily by
        lambda_mult * sim(query, row) - (1 - lambda_mult) * max sim(row, already picked), on the device.  Returns
        (distance float64 [B,k], rows int64 [B,k]) in selection order, NaN / -1 padded; lambda_mult = 1 is `search(k)`."""
        q = self._queries_2d(queries)
        B = q.shape[0]
        dist = np.empty((B, k), dtype=np.float64)
        rows = np.empty((B, k), dtype=np.int64)
        check(self._h, self._lib.mi355dr_search_mmr(self._h, ptr(q, ctypes.c_float), B, int(k), int(fetch_k), float(lambda_mult),
                                                    ptr(dist, ctypes.c_double), ptr(rows, ctypes.c_int64)))
        return dist, rows

    def search_mmr_device(self, q_ptr: int, B: int, k: int, fetch_k: int, out_dist_ptr: int, out_rows_ptr: int,
                          lambda_mult: float = 0.5, stream: int | None = None) -> None:
        """The same with queries and outputs in device memory; complete on return."""
        check(self._h, self._lib.mi355dr_search_mmr_device(
            self._h, ctypes.c_void_p(int(q_ptr)), int(B), int(k), int(fetch_k), float(lambda_mult),
            ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)),
            _stream_arg(stream)))

    def mmr_select(self, queries, k: int, cand_rows, lambda_mult: float = 0.5) -> tuple[np.ndarray, np.ndarray]:
        """MMR over each query's OWN candidate pool: cand_rows [B, m] global rows (m <= 1024) under the hygiene of
        `score_subset` / `search_subset` -- ids outside the index and -1 padding skipped, duplicates once, removed rows
        skipped, any order.  Each pool is scored, put into the search's order and picked from on the device."""
        q = self._queries_2d(queries)
        ids = np.ascontiguousarray(cand_rows, dtype=np.int64)
        if ids.ndim == 1:
            ids = ids[None, :]
        if ids.ndim != 2 or ids.shape[0] != q.shape[0]:
            raise ValueError(f"cand_rows must be [B, m] with B = {q.shape[0]}, got {ids.shape}")
        B = q.shape[0]
        dist = np.empty((B, k), dtype=np.float64)
        rows = np.empty((B, k), dtype=np.int64)
        check(self._h, self._lib.mi355dr_mmr_select(self._h, ptr(q, ctypes.c_float), B, int(k), ptr(ids, ctypes.c_int64),
                                                    ids.shape[1], float(lambda_mult), ptr(dist, ctypes.c_double),
                                                    ptr(rows, ctypes.c_int64)))
        return dist, rows

    # ---- grouped search: sub-query lists fused into one per group on the device (include/mi355dr.h "grouped search") ----
    @staticmethod
    def _group_offsets(group_offsets) -> np.ndarray:
        offs = np.ascontiguousarray(group_offsets, dtype=np.int32)
        if offs.ndim != 1 or offs.shape[0] < 1:
            raise ValueError("group_offsets must be one-dimensional [G + 1]")
        return offs

    def search_groups(self, queries, group_offsets, k: int, fetch_k: int | None = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Several searches per question, fused on the device: group g owns sub-queries group_offsets[g] ..
        group_offsets[g + 1] - 1 of `queries` [S, dim]; every sub-query is searched at `fetch_k` (default k) and the lists of
        a group become one -- every row once, at its smallest distance, in the order of `search`.  Returns (distance float64
        [G,k], rows int64 [G,k], count int32 [G] = distinct rows in the group's union); NaN / -1 padded."""
        offs = self._group_offsets(group_offsets)
        G = offs.shape[0] - 1
        q = f32c(queries)
        q = q.reshape(0, self.dim) if q.size == 0 else self._queries_2d(q)
        if q.shape[0] != int(offs[-1]):
            raise ValueError(f"group_offsets must end at the number of queries ({q.shape[0]}), got {int(offs[-1])}")
        fetch_k = int(k if fetch_k is None else fetch_k)
        dist = np.empty((G, k), dtype=np.float64)
        rows = np.empty((G, k), dtype=np.int64)
        count = np.empty(G, dtype=np.int32)
        check(self._h, self._lib.mi355dr_search_groups(self._h, ptr(q, ctypes.c_float), ptr(offs, ctypes.c_int32), G, int(k),
                                                       fetch_k, ptr(dist, ctypes.c_double), ptr(rows, ctypes.c_int64),
                                                       ptr(count, ctypes.c_int32)))
        return dist, rows, count

    def search_groups_device(self, q_ptr: int, group_offsets, k: int, fetch_k: int, out_dist_ptr: int, out_rows_ptr: int,
                             out_count_ptr: int | None = None, stream: int | None = None) -> None:
        """The same with queries ([group_offsets[-1], dim] fp32) and outputs (float64 [G,k], int64 [G,k], int32 [G] or
        None) in device memory; `group_offsets` stays on the host.  Complete on return."""
        offs = self._group_offsets(group_offsets)
        check(self._h, self._lib.mi355dr_search_groups_device(
            self._h, ctypes.c_void_p(int(q_ptr)), ptr(offs, ctypes.c_int32), offs.shape[0] - 1, int(k), int(fetch_k),
            ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)),
            ctypes.c_void_p(int(out_count_ptr) if out_count_ptr else None), _stream_arg(stream)))

    def merge_groups_device(self, vals_ptr: int, rows_ptr: int, S: int, width: int, group_offsets, k: int, out_vals_ptr: int,
                            out_rows_ptr: int, out_count_ptr: int | None = None, stream: int | None = None) -> None:
        """The merge alone over device lists (float64 / int64 [S, width]); `group_offsets` stays on the host."""
        offs = self._group_offsets(group_offsets)
        check(self._h, self._lib.mi355dr_merge_groups_device(
            self._h, ctypes.c_void_p(int(vals_ptr)), ctypes.c_void_p(int(rows_ptr)), int(S), int(width),
            ptr(offs, ctypes.c_int32), offs.shape[0] - 1, int(k), ctypes.c_void_p(int(out_vals_ptr)),
            ctypes.c_void_p(int(out_rows_ptr)), ctypes.c_void_p(int(out_count_ptr) if out_count_ptr else None),
            _stream_arg(stream)))

    def merge_groups(self, vals, rows, group_offsets, k: int, want_count: bool = True):
        """Fuse host lists on the device: vals float64 [S, width] (any doubles: distances, negated scores), rows int64
        [S, width] (-1 = no entry), group g = lists group_offsets[g] .. group_offsets[g + 1] - 1.  Every row once, at its
        smallest value (NaN last), sorted by (value, row); returns (vals [G,k], rows [G,k], count [G]) -- count is None with
        want_count=False (the kernel then writes none)."""
        v = np.ascontiguousarray(vals, dtype=np.float64)
        r = np.ascontiguousarray(rows, dtype=np.int64)
        if v.ndim != 2 or r.shape != v.shape:
            raise ValueError("vals and rows must both be [S, width]")
        offs = self._group_offsets(group_offsets)
        G, (S, width) = offs.shape[0] - 1, v.shape
        out_v = np.empty((G, k), dtype=np.float64)
        out_r = np.empty((G, k), dtype=np.int64)
        out_c = np.empty(G, dtype=np.int32) if want_count else None
        bufs = []
        try:
            for nbytes in (max(v.nbytes, 8), max(r.nbytes, 8), max(out_v.nbytes, 8), max(out_r.nbytes, 8), max(4 * G, 8)):
                bufs.append(self.dev_alloc(nbytes))
            if v.size:
                self.dev_upload(bufs[0], v)
                self.dev_upload(bufs[1], r)
            self.merge_groups_device(bufs[0], bufs[1], S, width, offs, k, bufs[2], bufs[3], bufs[4] if want_count else None)
            if G:
                self.dev_download(bufs[2], out_v)
                self.dev_download(bufs[3], out_r)
                if want_count:
                    self.dev_download(bufs[4], out_c)
        finally:
            for b in bufs:
                self.dev_free(b)
        return out_v, out_r, out_c

    # ---- hybrid fusion: two ranked lists per query fused into one on the device (include/mi355dr.h "hybrid fusion") ----
    @staticmethod
    def _fuse_opts(method: str, modes, rrf_k: int, fetch_k: int, weight: float, mins) -> "_native.FuseOpts":
        if method not in FUSE_METHODS:
            raise ValueError(f"method must be one of {sorted(FUSE_METHODS)}")
        if len(modes) != 2 or any(m not in FUSE_MODES for m in modes):
            raise ValueError(f"modes must be two of {sorted(FUSE_MODES)}")
        if method == "tmm" and (mins is None or len(mins) != 2 or any(m is None for m in mins)):
            raise ValueError("TMM normalization requires both minima")
        lo = (0.0, 0.0) if mins is None or method != "tmm" else mins
        return _native.FuseOpts(FUSE_METHODS[method], FUSE_MODES[modes[0]], FUSE_MODES[modes[1]], int(rrf_k), int(fetch_k),
                                float(weight), float(lo[0]), float(lo[1]))

    def fuse_lists_device(self, vals1_ptr: int, ids1_ptr: int, w1: int, vals2_ptr: int, ids2_ptr: int, w2: int, B: int, k: int,
                          out_vals_ptr: int, out_ids_ptr: int, out_count_ptr: int | None = None, *, method: str,
                          modes=("as_is", "as_is"), rrf_k: int = 60, fetch_k: int = 0, weight: float = 0.5, mins=None,
                          map1_ptr: int | None = None, map1_len: int = 0, map2_ptr: int | None = None, map2_len: int = 0,
                          stream: int | None = None) -> None:
        """The fusion over device lists (float64 / int64 [B, w_l]; maps int64 [map_len_l] or None; outputs float64 / int64
        [B, k] and int32 [B] or None).  It reads no index state: the lists may be another handle's.  Complete on return."""
        opts = self._fuse_opts(method, modes, rrf_k, fetch_k, weight, mins)
        vp = lambda p: ctypes.c_void_p(int(p) if p else None)  # noqa: E731
        check(self._h, self._lib.mi355dr_fuse_lists_device(
            self._h, vp(vals1_ptr), vp(ids1_ptr), int(w1), vp(map1_ptr), int(map1_len), vp(vals2_ptr), vp(ids2_ptr), int(w2),
            vp(map2_ptr), int(map2_len), int(B), int(k), ctypes.byref(opts), vp(out_vals_ptr), vp(out_ids_ptr), vp(out_count_ptr),
            _stream_arg(stream)))

    def fuse_lists(self, vals1, ids1, vals2, ids2, k: int, *, method: str, modes=("as_is", "as_is"), rrf_k: int = 60,
                   fetch_k: int = 0, weight: float = 0.5, mins=None, map1=None, map2=None):
        """Fuse two ranked lists per query on the device: vals_l float64 [B, w_l], ids_l int64 [B, w_l] (an id < 0, a NaN
        value, or an id its map strikes out is no entry), `modes` = how each list's values become scores ("one_minus": a
        cosine distance, "negate": a BM25 distance, "as_is").  method "rrf" (rrf_k, fetch_k) or a convex combination "mm" |
        "tmm" | "z" | "dbsf" (weight; mins for tmm) -- hybrid.rrf_fuse / hybrid.cc_fuse over first-seen order.  map_l: int64
        array translating list l's ids into the common id space.  Returns (scores [B,k], ids [B,k], count int32 [B] = size of
        each union); NaN / -1 padded."""
        v1 = np.ascontiguousarray(vals1, dtype=np.float64)
        i1 = np.ascontiguousarray(ids1, dtype=np.int64)
        v2 = np.ascontiguousarray(vals2, dtype=np.float64)
        i2 = np.ascontiguousarray(ids2, dtype=np.int64)
        if v1.ndim != 2 or i1.shape != v1.shape or v2.ndim != 2 or i2.shape != v2.shape or v1.shape[0] != v2.shape[0]:
            raise ValueError("vals_l and ids_l must both be [B, w_l] with one B")
        maps = [None if m is None else np.ascontiguousarray(m, dtype=np.int64).reshape(-1) for m in (map1, map2)]
        opts = self._fuse_opts(method, modes, rrf_k, fetch_k, weight, mins)
        B, k = v1.shape[0], int(k)
        out_v = np.empty((B, max(k, 0)), dtype=np.float64)
        out_i = np.empty((B, max(k, 0)), dtype=np.int64)
        out_c = np.empty(B, dtype=np.int32)
        mp = lambda m: (None, 0) if m is None else (ptr(m, ctypes.c_int64), m.shape[0])  # noqa: E731
        check(self._h, self._lib.mi355dr_fuse_lists(
            self._h, ptr(v1, ctypes.c_double), ptr(i1, ctypes.c_int64), v1.shape[1], *mp(maps[0]), ptr(v2, ctypes.c_double),
            ptr(i2, ctypes.c_int64), v2.shape[1], *mp(maps[1]), B, k, ctypes.byref(opts), ptr(out_v, ctypes.c_double),
            ptr(out_i, ctypes.c_int64), ptr(out_c, ctypes.c_int32)))
        return out_v, out_i, out_c

    # ---- source-capped lists and search: at most `cap` results per source (include/mi355dr.h "source-capped lists and search") ----
    def upload_keys(self, keys) -> "DeviceKeys":
        """A key table (int64 [keys_len], keys[id] = the source of id, negative = none) uploaded ONCE, for any number of
        `collapse_lists` / `search_collapsed*` calls; close it (or use it as a context manager) when done.  A numpy table
        passed per call takes the host form instead, which uploads it every time."""
        return DeviceKeys(self, keys)

    @staticmethod
    def _host_keys(keys) -> np.ndarray | None:
        if keys is None:
            return None
        t = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        return t if t.shape[0] else None   # (an empty table gives no entry a key: the C ABI's NULL / 0)

    def collapse_lists_device(self, vals_ptr: int, ids_ptr: int, w: int, B: int, cap: int, k: int, out_vals_ptr: int,
                              out_ids_ptr: int, out_keys_ptr: int | None = None, out_pos_ptr: int | None = None,
                              out_count_ptr: int | None = None, out_entries_ptr: int | None = None, *,
                              keys_ptr: int | None = None, keys_len: int = 0, stream: int | None = None) -> None:
        """The cap over device lists (float64 / int64 [B, w]; table int64 [keys_len] or None; outputs float64 / int64 [B, k],
        and each of int64 [B, k] keys, int32 [B, k] positions, int32 [B] kept, int32 [B] entries or None).  It reads no
        index state: the lists may be another handle's.  Complete on return."""
        vp = lambda p: ctypes.c_void_p(int(p) if p else None)  # noqa: E731
        check(self._h, self._lib.mi355dr_collapse_lists_device(
            self._h, vp(vals_ptr), vp(ids_ptr), int(w), int(B), vp(keys_ptr), int(keys_len), int(cap), int(k), vp(out_vals_ptr),
            vp(out_ids_ptr), vp(out_keys_ptr), vp(out_pos_ptr), vp(out_count_ptr), vp(out_entries_ptr), _stream_arg(stream)))

    def collapse_lists(self, vals, ids, keys, cap: int, k: int | None = None, *, with_keys: bool = True, with_pos: bool = True,
                       with_count: bool = True, with_entries: bool = True) -> "CollapsedLists":
        """At most `cap` entries per source in each ranked list: vals float64 [B, w], ids int64 [B, w] in ranking order (an
        id < 0 is no entry; a NaN value with an id is one).  `keys`: None, an int64 array (the host form) or a `DeviceKeys`
        (`upload_keys`: the device form).  An entry is kept iff it has no key or fewer than `cap` earlier entries of its list
        have its key; the first `k` (default w) kept entries come back in list order with the bits they came with, NaN / -1
        behind them.  Returns CollapsedLists(vals [B,k], ids [B,k], keys [B,k] (-1: none), pos int32 [B,k] (slot in the
        input), count int32 [B] (kept in the whole list), entries int32 [B]); a field switched off is None."""
        v = np.ascontiguousarray(vals, dtype=np.float64)
        i = np.ascontiguousarray(ids, dtype=np.int64)
        if v.ndim != 2 or i.shape != v.shape:
            raise ValueError("vals and ids must both be [B, w]")
        B, w = v.shape
        k = int(w if k is None else k)
        out_v = np.empty((B, max(k, 0)), dtype=np.float64)
        out_i = np.empty((B, max(k, 0)), dtype=np.int64)
        out_k = np.empty((B, max(k, 0)), dtype=np.int64) if with_keys else None
        out_p = np.empty((B, max(k, 0)), dtype=np.int32) if with_pos else None
        out_c = np.empty(B, dtype=np.int32) if with_count else None
        out_e = np.empty(B, dtype=np.int32) if with_entries else None
        outs = (out_v, out_i, out_k, out_p, out_c, out_e)
        if isinstance(keys, DeviceKeys):
            bufs = []
            try:
                for a in (v, i, *outs):
                    bufs.append(None if a is None else self.dev_alloc(max(a.nbytes, 8)))
                if v.size:
                    self.dev_upload(bufs[0], v)
                    self.dev_upload(bufs[1], i)
                self.collapse_lists_device(bufs[0], bufs[1], w, B, cap, k, *bufs[2:], keys_ptr=keys.ptr, keys_len=keys.length)
                for a, b in zip(outs, bufs[2:]):
                    if a is not None and a.size:
                        self.dev_download(b, a)
            finally:
                for b in bufs:
                    if b is not None:
                        self.dev_free(b)
            return CollapsedLists(*outs)
        t = self._host_keys(keys)
        opt = lambda a, ct: None if a is None else ptr(a, ct)  # noqa: E731
        check(self._h, self._lib.mi355dr_collapse_lists(
            self._h, ptr(v, ctypes.c_double), ptr(i, ctypes.c_int64), int(w), B, opt(t, ctypes.c_int64),
            0 if t is None else t.shape[0], int(cap), k, ptr(out_v, ctypes.c_double), ptr(out_i, ctypes.c_int64),
            opt(out_k, ctypes.c_int64), opt(out_p, ctypes.c_int32), opt(out_c, ctypes.c_int32), opt(out_e, ctypes.c_int32)))
        return CollapsedLists(*outs)

    @staticmethod
    def collapse_fetch_k(k: int, fetch_k: int | None, max_fetch: int) -> int:
        """The first round's width of `search_collapsed*`: `fetch_k`, or COLLAPSE_FETCH_MULT * k within [k, max_fetch]."""
        if fetch_k is not None:
            return int(fetch_k)
        return max(int(k), min(COLLAPSE_FETCH_MULT * int(k), int(max_fetch)))

    def _search_collapsed_device_form(self, fn, q_ptr: int, B: int, k: int, cap: int, keys_ptr, keys_len: int, fetch_k: int,
                                      max_fetch: int, out_dist_ptr: int, out_rows_ptr: int, out_keys_ptr, out_count_ptr,
                                      out_state_ptr, stream) -> None:
        vp = lambda p: ctypes.c_void_p(int(p) if p else None)  # noqa: E731
        check(self._h, fn(self._h, vp(q_ptr), int(B), int(k), int(cap), vp(keys_ptr), int(keys_len), int(fetch_k), int(max_fetch),
                          vp(out_dist_ptr), vp(out_rows_ptr), vp(out_keys_ptr), vp(out_count_ptr), vp(out_state_ptr),
                          _stream_arg(stream)))

    def search_collapsed_device(self, q_ptr: int, B: int, k: int, cap: int, fetch_k: int, max_fetch: int, out_dist_ptr: int,
                                out_rows_ptr: int, out_keys_ptr: int | None = None, out_count_ptr: int | None = None,
                                out_state_ptr: int | None = None, *, keys_ptr: int | None = None, keys_len: int = 0,
                                stream: int | None = None) -> None:
        """`search_collapsed` with queries, table and outputs (float64 / int64 / int64 [B, k], int32 [B] count and state) in
        device memory; complete on return."""
        self._search_collapsed_device_form(self._lib.mi355dr_search_collapsed_device, q_ptr, B, k, cap, keys_ptr, keys_len,
                                           fetch_k, max_fetch, out_dist_ptr, out_rows_ptr, out_keys_ptr, out_count_ptr,
                                           out_state_ptr, stream)

    def search_collapsed_sharded_device(self, q_ptr: int, B: int, k: int, cap: int, fetch_k: int, max_fetch: int,
                                        out_dist_ptr: int, out_rows_ptr: int, out_keys_ptr: int | None = None,
                                        out_count_ptr: int | None = None, out_state_ptr: int | None = None, *,
                                        keys_ptr: int | None = None, keys_len: int = 0, stream: int | None = None) -> None:
        """The same over the communicator: every rank passes the same arguments (the table is indexed by GLOBAL rows) and
        receives what one index holding all rows would return."""
        self._search_collapsed_device_form(self._lib.mi355dr_search_collapsed_sharded_device, q_ptr, B, k, cap, keys_ptr,
                                           keys_len, fetch_k, max_fetch, out_dist_ptr, out_rows_ptr, out_keys_ptr,
                                           out_count_ptr, out_state_ptr, stream)

    def _search_collapsed_buffers(self, device_form, queries, k: int, cap: int, keys, fetch_k: int,
                                  max_fetch: int) -> "CollapsedSearch":
        """One call of a _device form over buffers of this call: the queries uploaded, the five results downloaded; a numpy
        table is uploaded for the call, a DeviceKeys is used in place."""
        q, qp = self._device_queries(queries)
        B, k = q.shape[0], int(k)
        outs = (np.empty((B, max(k, 0)), dtype=np.float64), np.empty((B, max(k, 0)), dtype=np.int64),
                np.empty((B, max(k, 0)), dtype=np.int64), np.empty(B, dtype=np.int32), np.empty(B, dtype=np.int32))
        own = None if keys is None or isinstance(keys, DeviceKeys) else DeviceKeys(self, keys)
        table = own if own is not None else keys
        bufs = []
        try:
            for a in outs:
                bufs.append(self.dev_alloc(max(a.nbytes, 8)))
            device_form(qp, B, k, cap, fetch_k, max_fetch, *bufs, keys_ptr=table.ptr if table is not None else None,
                        keys_len=table.length if table is not None else 0)
            for a, b in zip(outs, bufs):
                if a.size:
                    self.dev_download(b, a)
        finally:
            for b in bufs:
                self.dev_free(b)
            self.dev_free(qp)
            if own is not None:
                own.close()
        return CollapsedSearch(*outs)

    def search_collapsed(self, queries, k: int, cap: int, keys, fetch_k: int | None = None,
                         max_fetch: int = 1024) -> "CollapsedSearch":
        """The best `k`, at most `cap` per source: `search` whose ranking is walked under the cap.  keys: int64 [keys_len]
        indexed by the rows `search` returns (negative or beyond the table: no source, never capped), a `DeviceKeys`, or None
        (the bits of `search(queries, k)`).  The block is searched at `fetch_k` and only the queries whose cap bit deeper
        are searched again, at twice the width, up to `max_fetch` <= 1024: the result is that of one pass at `max_fetch`
        whatever `fetch_k` is (default: `collapse_fetch_k`).  Returns CollapsedSearch(dist float64 [B,k], rows int64 [B,k],
        keys int64 [B,k] (-1: none), count int32 [B] (lines written), state int32 [B] (COLLAPSE_TRUNCATED: fewer than k
        although the ranking was cut at max_fetch)); NaN / -1 padded."""
        f = self.collapse_fetch_k(k, fetch_k, max_fetch)
        if isinstance(keys, DeviceKeys):
            return self._search_collapsed_buffers(self.search_collapsed_device, queries, k, cap, keys, f, max_fetch)
        q = self._queries_2d(queries)
        t = self._host_keys(keys)
        B, k = q.shape[0], int(k)
        dist = np.empty((B, max(k, 0)), dtype=np.float64)
        rows = np.empty((B, max(k, 0)), dtype=np.int64)
        okeys = np.empty((B, max(k, 0)), dtype=np.int64)
        count = np.empty(B, dtype=np.int32)
        state = np.empty(B, dtype=np.int32)
        check(self._h, self._lib.mi355dr_search_collapsed(
            self._h, ptr(q, ctypes.c_float), B, k, int(cap), None if t is None else ptr(t, ctypes.c_int64),
            0 if t is None else t.shape[0], f, int(max_fetch), ptr(dist, ctypes.c_double), ptr(rows, ctypes.c_int64),
            ptr(okeys, ctypes.c_int64), ptr(count, ctypes.c_int32), ptr(state, ctypes.c_int32)))
        return CollapsedSearch(dist, rows, okeys, count, state)

    def search_collapsed_sharded(self, queries, k: int, cap: int, keys, fetch_k: int | None = None,
                                 max_fetch: int = 1024) -> "CollapsedSearch":
        """`search_collapsed` over the shards; `keys` is indexed by global rows and is the same on every rank."""
        f = self.collapse_fetch_k(k, fetch_k, max_fetch)
        return self._search_collapsed_buffers(self.search_collapsed_sharded_device, queries, k, cap, keys, f, max_fetch)

    def search_maxsim_collapsed(self, qtok, q_offsets, k: int, cap: int, keys, fetch_k: int):
        """`search_maxsim` at `fetch_k`, then the cap over its lists (`collapse_lists`): at most `cap` documents per source
        among the first `fetch_k`.  The fp32 distances are taken from the search's own list through the kept entries'
        positions, so their bits are the search's.  Returns (distance float32 [B,k], docs int64 [B,k], keys int64 [B,k],
        count int32 [B] = kept among the fetch_k)."""
        dist, docs = self.search_maxsim(qtok, q_offsets, int(fetch_k))
        got = self.collapse_lists(dist.astype(np.float64), docs, keys, cap, k, with_entries=False)
        out = np.full(got.pos.shape, np.nan, dtype=np.float32)
        b, s = np.nonzero(got.pos >= 0)
        out[b, s] = dist[b, got.pos[b, s]]
        return out, got.ids, got.keys, got.count

    def search_bm25_collapsed(self, token_lists, k: int, cap: int, keys, fetch_k: int, k1: float = 1.2, b: float = 0.75,
                              offsets=None):
        """`search_bm25` at `fetch_k`, then the cap over its lists: at most `cap` documents per source among the first
        `fetch_k`.  Returns (distance float64 [B,k] = -score, ids int64 [B,k], keys int64 [B,k], count int32 [B])."""
        dist, ids = self.search_bm25(token_lists, int(fetch_k), k1, b, offsets=offsets)
        got = self.collapse_lists(dist, ids, keys, cap, k, with_pos=False, with_entries=False)
        return got.vals, got.ids, got.keys, got.count

    # ---- range search: every row within a distance, counted on the device (include/mi355dr.h "range search") ----
    @staticmethod
    def _radius(radius, B: int) -> np.ndarray:
        """A scalar or a [B] array -> float64 [B]; NaN and any other shape are refused before the library is called."""
        r = np.asarray(radius, dtype=np.float64)
        if r.ndim == 0:
            r = np.full(B, float(r), dtype=np.float64)
        if r.ndim != 1 or r.shape[0] != B:
            raise ValueError(f"radius must be a scalar or one-dimensional [{B}], got shape {r.shape}")
        if np.isnan(r).any():
            raise ValueError("radius must not be NaN")
        return np.ascontiguousarray(r)

    def search_range(self, queries, radius, max_results: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`WHERE distance <= radius ORDER BY distance LIMIT max_results`, and `count(*)` under the same filter.  `radius`: a
        scalar or [B], in the metric's distance units (cosine distance; -dot for "ip"); +inf = every row with a defined
        distance.  Returns (distance float64 [B,m], rows int64 [B,m], count int64 [B]): the first min(count, m) in-range rows
        in the order of `search`, with its bits, NaN / -1 behind them; count is exact and may exceed m."""
        q = self._queries_2d(queries)
        B, m = q.shape[0], int(max_results)
        r = self._radius(radius, B)
        dist = np.empty((B, max(m, 0)), dtype=np.float64)
        rows = np.empty((B, max(m, 0)), dtype=np.int64)
        count = np.empty(B, dtype=np.int64)
        check(self._h, self._lib.mi355dr_search_range(self._h, ptr(q, ctypes.c_float), B, ptr(r, ctypes.c_double), m,
                                                      ptr(dist, ctypes.c_double), ptr(rows, ctypes.c_int64),
                                                      ptr(count, ctypes.c_int64)))
        return dist, rows, count

    def search_range_device(self, q_ptr: int, B: int, radius, max_results: int, out_dist_ptr: int, out_rows_ptr: int,
                            out_count_ptr: int, stream: int | None = None) -> None:
        """The same with queries ([B, dim] fp32) and outputs (float64 [B,m], int64 [B,m], int64 [B]) in device memory; the
        radii stay on the host.  Complete on return."""
        r = self._radius(radius, int(B))
        check(self._h, self._lib.mi355dr_search_range_device(
            self._h, ctypes.c_void_p(int(q_ptr)), int(B), ptr(r, ctypes.c_double), int(max_results),
            ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)), ctypes.c_void_p(int(out_count_ptr)),
            _stream_arg(stream)))

    # ---- search by stored row: neighbours of rows, self excluded (include/mi355dr.h "search by stored row") ----
    def search_rows(self, row_ids, k: int, include_self: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """The top-k of the stored rows `row_ids` (global ids, any order, repeats allowed), the query vectors read on the
        device.  By default the row itself is left out: the top-k of the OTHER live rows, in the order and with the bits of
        `search`; include_self=True is `search(get_rows(row_ids), k)`.  An id outside the index and a removed row give a
        NaN / -1 line.  Returns (distance float64 [B,k], rows int64 [B,k])."""
        ids = self._row_ids(row_ids)
        B = ids.shape[0]
        dist = np.empty((B, max(int(k), 0)), dtype=np.float64)
        rows = np.empty((B, max(int(k), 0)), dtype=np.int64)
        check(self._h, self._lib.mi355dr_search_rows(self._h, ptr(ids, ctypes.c_int64), B, int(k), 1 if include_self else 0,
                                                     ptr(dist, ctypes.c_double), ptr(rows, ctypes.c_int64)))
        return dist, rows

    def search_rows_device(self, row_ids, k: int, out_dist_ptr: int, out_rows_ptr: int, include_self: bool = False,
                           stream: int | None = None) -> None:
        """The same with the outputs (float64 / int64 [B,k]) in device memory; the ids stay on the host.  Complete on return."""
        ids = self._row_ids(row_ids)
        check(self._h, self._lib.mi355dr_search_rows_device(
            self._h, ptr(ids, ctypes.c_int64), ids.shape[0], int(k), 1 if include_self else 0, ctypes.c_void_p(int(out_dist_ptr)),
            ctypes.c_void_p(int(out_rows_ptr)), _stream_arg(stream)))

    def search_range_rows(self, row_ids, radius, max_results: int,
                          include_self: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`search_range` with the stored rows `row_ids` as queries; by default the row itself is left out of the count and
        of the list.  Returns (distance float64 [B,m], rows int64 [B,m], count int64 [B]); count is exact and may exceed m."""
        ids = self._row_ids(row_ids)
        B, m = ids.shape[0], int(max_results)
        r = self._radius(radius, B)
        dist = np.empty((B, max(m, 0)), dtype=np.float64)
        rows = np.empty((B, max(m, 0)), dtype=np.int64)
        count = np.empty(B, dtype=np.int64)
        check(self._h, self._lib.mi355dr_search_range_rows(
            self._h, ptr(ids, ctypes.c_int64), B, ptr(r, ctypes.c_double), m, 1 if include_self else 0,
            ptr(dist, ctypes.c_double), ptr(rows, ctypes.c_int64), ptr(count, ctypes.c_int64)))
        return dist, rows, count

    def search_range_rows_device(self, row_ids, radius, max_results: int, out_dist_ptr: int, out_rows_ptr: int,
                                 out_count_ptr: int, include_self: bool = False, stream: int | None = None) -> None:
        """The same with the three outputs in device memory; ids and radii stay on the host.  Complete on return."""
        ids = self._row_ids(row_ids)
        r = self._radius(radius, ids.shape[0])
        check(self._h, self._lib.mi355dr_search_range_rows_device(
            self._h, ptr(ids, ctypes.c_int64), ids.shape[0], ptr(r, ctypes.c_double), int(max_results),
            1 if include_self else 0, ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)),
            ctypes.c_void_p(int(out_count_ptr)), _stream_arg(stream)))

    # ---- search by examples / feedback: queries built on the device (include/mi355dr.h "search by examples / feedback") ----
    @staticmethod
    def _example_lists(lists, B: int | None) -> np.ndarray:
        """Example ids -> int64 [B, m], -1 padded.  None: no examples; a flat sequence of ids: one slot; a sequence of
        sequences (ragged allowed): one list per slot."""
        if lists is None:
            return np.full((B or 0, 0), -1, dtype=np.int64)
        if isinstance(lists, np.ndarray):
            a = np.ascontiguousarray(lists, dtype=np.int64)
            if a.ndim == 1:
                a = a[None, :]
        else:
            lists = list(lists)
            if not lists:
                return np.full((B or 0, 0), -1, dtype=np.int64)
            if all(np.ndim(x) == 0 for x in lists):
                lists = [lists]
            m = max((len(x) for x in lists), default=0)
            a = np.full((len(lists), m), -1, dtype=np.int64)
            for b, x in enumerate(lists):
                a[b, :len(x)] = np.asarray(x, dtype=np.int64)
        if a.ndim != 2 or (B is not None and a.shape[0] != B):
            raise ValueError(f"example ids must be [B, m] with B = {B}, got shape {a.shape}")
        return a

    def _example_args(self, queries, pos_ids, neg_ids):
        q = None if queries is None else self._queries_2d(queries)
        pos = self._example_lists(pos_ids, None if q is None else q.shape[0])
        B = pos.shape[0] if q is None else q.shape[0]
        neg = self._example_lists(neg_ids, B)
        return q, B, pos, neg

    @staticmethod
    def _ids_arg(a: np.ndarray):
        return ptr(a, ctypes.c_int64) if a.size else None

    def combine_rows(self, pos_ids, neg_ids=None, queries=None, alpha: float = 1.0, beta: float = 1.0,
                     gamma: float = 1.0) -> tuple[np.ndarray, np.ndarray]:
        """Per slot alpha * base + beta * mean(positives) - gamma * mean(negatives) over stored rows (global ids, ragged lists
        are padded with -1), unit-normalised terms on a cosine index, formed on the device under the fixed double arithmetic
        of the header.  `queries`: the base vectors [B, dim] or None.  Returns (vectors float32 [B, dim], valid int32 [B]);
        beta = 1 without a base and without negatives is the centroid of the listed rows."""
        q, B, pos, neg = self._example_args(queries, pos_ids, neg_ids)
        vec = np.empty((B, self.dim), dtype=np.float32)
        valid = np.empty(B, dtype=np.int32)
        check(self._h, self._lib.mi355dr_combine_rows(
            self._h, None if q is None else ptr(q, ctypes.c_float), B, self._ids_arg(pos), pos.shape[1], self._ids_arg(neg),
            neg.shape[1], float(alpha), float(beta), float(gamma), ptr(vec, ctypes.c_float), ptr(valid, ctypes.c_int32)))
        return vec, valid

    def combine_rows_device(self, pos_ids, neg_ids, q_ptr: int | None, out_vectors_ptr: int, out_valid_ptr: int,
                            alpha: float = 1.0, beta: float = 1.0, gamma: float = 1.0, stream: int | None = None) -> None:
        """The same with the base vectors (or None) and both outputs in device memory; the ids stay on the host."""
        pos = self._example_lists(pos_ids, None)
        neg = self._example_lists(neg_ids, pos.shape[0])
        check(self._h, self._lib.mi355dr_combine_rows_device(
            self._h, ctypes.c_void_p(int(q_ptr)) if q_ptr else None, pos.shape[0], self._ids_arg(pos), pos.shape[1],
            self._ids_arg(neg), neg.shape[1], float(alpha), float(beta), float(gamma), ctypes.c_void_p(int(out_vectors_ptr)),
            ctypes.c_void_p(int(out_valid_ptr)), _stream_arg(stream)))

    def search_examples(self, pos_ids, k: int, neg_ids=None, queries=None, alpha: float = 1.0, beta: float = 1.0,
                        gamma: float = 1.0, keep: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """"More like these, less like those": `search(combine_rows(...), k)` with every listed row left out of the answer
        (keep=True: nothing is left out), in one call on the device.  Returns (distance float64 [B,k], rows int64 [B,k]); an
        invalid slot (`combine_rows`) gives a NaN / -1 line."""
        q, B, pos, neg = self._example_args(queries, pos_ids, neg_ids)
        dist = np.empty((B, max(int(k), 0)), dtype=np.float64)
        rows = np.empty((B, max(int(k), 0)), dtype=np.int64)
        check(self._h, self._lib.mi355dr_search_examples(
            self._h, None if q is None else ptr(q, ctypes.c_float), B, self._ids_arg(pos), pos.shape[1], self._ids_arg(neg),
            neg.shape[1], float(alpha), float(beta), float(gamma), int(k), 1 if keep else 0, ptr(dist, ctypes.c_double),
            ptr(rows, ctypes.c_int64)))
        return dist, rows

    def search_examples_device(self, pos_ids, neg_ids, q_ptr: int | None, k: int, out_dist_ptr: int, out_rows_ptr: int,
                               alpha: float = 1.0, beta: float = 1.0, gamma: float = 1.0, keep: bool = False,
                               stream: int | None = None) -> None:
        """The same with the base vectors (or None) and the outputs (float64 / int64 [B,k]) in device memory; the ids stay on
        the host.  Complete on return."""
        pos = self._example_lists(pos_ids, None)
        neg = self._example_lists(neg_ids, pos.shape[0])
        check(self._h, self._lib.mi355dr_search_examples_device(
            self._h, ctypes.c_void_p(int(q_ptr)) if q_ptr else None, pos.shape[0], self._ids_arg(pos), pos.shape[1],
            self._ids_arg(neg), neg.shape[1], float(alpha), float(beta), float(gamma), int(k), 1 if keep else 0,
            ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)), _stream_arg(stream)))

    def search_feedback(self, queries, k: int, fb_k: int = 10, alpha: float = 1.0,
                        beta: float = 0.75) -> tuple[np.ndarray, np.ndarray]:
        """Rocchio pseudo-relevance feedback: `search` at `fb_k`, the query moved towards the mean of those rows
        (alpha * query + beta * mean, `combine_rows`), `search` of the moved query at `k`.  The first pass's lists never
        leave the device.  Returns (distance float64 [B,k], rows int64 [B,k])."""
        q = self._queries_2d(queries)
        B = q.shape[0]
        dist = np.empty((B, max(int(k), 0)), dtype=np.float64)
        rows = np.empty((B, max(int(k), 0)), dtype=np.int64)
        check(self._h, self._lib.mi355dr_search_feedback(self._h, ptr(q, ctypes.c_float), B, int(k), int(fb_k), float(alpha),
                                                         float(beta), ptr(dist, ctypes.c_double), ptr(rows, ctypes.c_int64)))
        return dist, rows

    def search_feedback_device(self, q_ptr: int, B: int, k: int, fb_k: int, out_dist_ptr: int, out_rows_ptr: int,
                               alpha: float = 1.0, beta: float = 0.75, stream: int | None = None) -> None:
        """The same with queries and outputs in device memory; complete on return."""
        check(self._h, self._lib.mi355dr_search_feedback_device(
            self._h, ctypes.c_void_p(int(q_ptr)), int(B), int(k), int(fb_k), float(alpha), float(beta),
            ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)), _stream_arg(stream)))

    def _row_span(self, row0: int, row1: int | None, block: int) -> tuple[int, int, int]:
        row0, row1, block = int(row0), len(self) if row1 is None else int(row1), int(block)
        if row1 < row0 or block < 1:
            raise ValueError("need row0 <= row1 and block >= 1")
        return row0, row1, block

    def knn_graph(self, k: int, row0: int = 0, row1: int | None = None, block: int = 1024) -> tuple[np.ndarray, np.ndarray]:
        """The exact k-NN graph of rows row0 .. row1-1 (global ids; row1=None: len(self)): line i holds the k nearest OTHER
        live rows of row row0 + i, from `search_rows` in blocks of `block` ids.  Removed rows give NaN / -1 lines.  Returns
        (distance float64 [n,k], rows int64 [n,k]); the rows never leave the device."""
        row0, row1, block = self._row_span(row0, row1, block)
        dist = np.empty((row1 - row0, int(k)), dtype=np.float64)
        rows = np.empty((row1 - row0, int(k)), dtype=np.int64)
        for a in range(row0, row1, block):
            b = min(a + block, row1)
            dist[a - row0:b - row0], rows[a - row0:b - row0] = self.search_rows(np.arange(a, b, dtype=np.int64), k)
        return dist, rows

    def near_duplicates(self, radius, max_results: int = 10, row0: int = 0, row1: int | None = None,
                        block: int = 1024) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """For rows row0 .. row1-1 (global ids; row1=None: len(self)) the OTHER live rows within `radius` (a scalar), from
        `search_range_rows` in blocks of `block` ids.  Returns (distance [n,m], rows [n,m], count [n]); count[i] > 0 means
        row row0 + i has a near-copy.  Removed rows give NaN / -1 lines and count 0."""
        row0, row1, block = self._row_span(row0, row1, block)
        m = int(max_results)
        dist = np.empty((row1 - row0, m), dtype=np.float64)
        rows = np.empty((row1 - row0, m), dtype=np.int64)
        count = np.empty(row1 - row0, dtype=np.int64)
        for a in range(row0, row1, block):
            b = min(a + block, row1)
            s = slice(a - row0, b - row0)
            dist[s], rows[s], count[s] = self.search_range_rows(np.arange(a, b, dtype=np.int64), float(radius), m)
        return dist, rows, count

    # ---- views: a listed subset as an index of its own (include/mi355dr.h "views") ----
    def view(self, row_ids=None, doc_ids=None) -> "Mi355Index":
        """The listed rows and / or documents of this index as a read-only index of their own, built on the device
        (mi355dr_view_create).  Ids are global, under the hygiene of `search_subset` (out-of-range ids and -1 padding skipped,
        duplicates once, any order); removed rows and documents without vectors are left out.  Every search of the view --
        `search`, `search_device*`, `search_maxsim*` -- runs the ordinary paths, screens included, and returns THIS index's
        ids: `view.search(Q, k)` equals `search_subset(Q, k, row_ids)` bit for bit.  The view is a snapshot (later changes
        here do not reach it, it outlives this index) and is closed on its own.  Worth it when one list serves many query
        blocks; a one-off list is cheaper through `search_subset`."""
        if not self._h:
            raise ValueError("view() on a closed index")
        rows = self._row_ids(() if row_ids is None else row_ids)
        docs = self._row_ids(() if doc_ids is None else doc_ids)
        h = ctypes.c_void_p()
        check(self._h, self._lib.mi355dr_view_create(self._h, ptr(rows, ctypes.c_int64), rows.shape[0],
                                                     ptr(docs, ctypes.c_int64), docs.shape[0], ctypes.byref(h)))
        v = object.__new__(type(self))
        v._lib, v._h, v.dim, v.metric, v.device, v._is_view = self._lib, h, self.dim, self.metric, self.device, True
        return v

    @property
    def is_view(self) -> bool:
        """True for an index returned by `view`: read-only, rows and documents named by the parent's ids."""
        return self._is_view

    def merge_topk_device(self, dist_all_ptr: int, rows_all_ptr: int, world: int, B: int, k: int, out_dist_ptr: int,
                          out_rows_ptr: int, stream: int | None = None) -> None:
        check(self._h, self._lib.mi355dr_merge_topk_device(
            self._h, ctypes.c_void_p(int(dist_all_ptr)), ctypes.c_void_p(int(rows_all_ptr)), int(world), int(B),
            int(k), ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)),
            _stream_arg(stream)))

    def pack_topk_device(self, dist_ptr: int, rows_ptr: int, B: int, k: int, packed_ptr: int, stream: int | None = None) -> None:
        check(self._h, self._lib.mi355dr_pack_topk_device(self._h, ctypes.c_void_p(int(dist_ptr)), ctypes.c_void_p(int(rows_ptr)),
                                                          int(B), int(k), ctypes.c_void_p(int(packed_ptr)),
                                                          _stream_arg(stream)))

    def merge_topk_packed_device(self, packed_all_ptr: int, world: int, B: int, k: int, out_dist_ptr: int, out_rows_ptr: int,
                                 stream: int | None = None) -> None:
        check(self._h, self._lib.mi355dr_merge_topk_packed_device(
            self._h, ctypes.c_void_p(int(packed_all_ptr)), int(world), int(B), int(k), ctypes.c_void_p(int(out_dist_ptr)),
            ctypes.c_void_p(int(out_rows_ptr)), _stream_arg(stream)))

    # ---- row-sharded search inside the library (RCCL, no torch): include/mi355dr.h "row-sharded search" ----
    @staticmethod
    def comm_unique_id() -> bytes:
        """128-byte ncclUniqueId (call on ONE rank, hand it to every rank through the host's own channel)."""
        from ._native import load

        buf = ctypes.create_string_buffer(128)
        check(None, load().mi355dr_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p), 128))
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: bytes) -> None:
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        check(self._h, self._lib.mi355dr_comm_init(self._h, int(rank), int(world), ctypes.cast(buf, ctypes.c_void_p), 128))

    def comm_init_custom(self, rank: int, world: int, all_gather) -> None:
        """The sharded search over the HOST's own all-gather instead of RCCL (mi355dr_comm_init_custom).
        `all_gather(send_ptr, recv_ptr, bytes_per_rank, stream_handle) -> None` moves device memory: every rank's
        `bytes_per_rank` bytes at `send_ptr` into `recv_ptr`, rank-major, complete on return (or ordered on the stream).
        An exception inside it becomes error code 1 of the search that called it."""
        from ._native import ALLGATHER_FN

        def thunk(send, recv, nbytes, stream, _user):
            try:
                all_gather(int(send or 0), int(recv or 0), int(nbytes), int(stream or 0))
            except Exception:  # noqa: BLE001 - must not unwind through the C frame
                import traceback

                traceback.print_exc()
                return 1
            return 0

        self._allgather_thunk = ALLGATHER_FN(thunk)   # (kept alive as long as the index may call it)
        check(self._h, self._lib.mi355dr_comm_init_custom(self._h, int(rank), int(world), self._allgather_thunk, None))

    def comm_world(self) -> int:
        return int(self._lib.mi355dr_comm_world(self._h))

    def comm_count(self) -> int:
        """Ranks RCCL itself reports for this index's communicator (ncclCommCount); 0 before comm_init."""
        n = ctypes.c_int(0)
        check(self._h, self._lib.mi355dr_comm_count(self._h, ctypes.byref(n)))
        return int(n.value)

    def search_sharded_device(self, q_ptr: int, B: int, k: int, out_dist_ptr: int, out_rows_ptr: int,
                              stream: int | None = None) -> None:
        """Local search + ONE ncclAllGather + merge, on device buffers (every rank: same queries in, same result out)."""
        check(self._h, self._lib.mi355dr_search_sharded_device(
            self._h, ctypes.c_void_p(int(q_ptr)), int(B), int(k), ctypes.c_void_p(int(out_dist_ptr)),
            ctypes.c_void_p(int(out_rows_ptr)), _stream_arg(stream)))

    # ---- the derived searches over the row-sharded index (include/mi355dr.h "the derived searches over a row-sharded index"):
    # every rank passes the same arguments and receives what one index holding all rows would return; complete on return ----
    def search_range_sharded_device(self, q_ptr: int, B: int, radius, max_results: int, out_dist_ptr: int, out_rows_ptr: int,
                                    out_count_ptr: int, stream: int | None = None) -> None:
        r = self._radius(radius, int(B))
        check(self._h, self._lib.mi355dr_search_range_sharded_device(
            self._h, ctypes.c_void_p(int(q_ptr)), int(B), ptr(r, ctypes.c_double), int(max_results),
            ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)), ctypes.c_void_p(int(out_count_ptr)),
            _stream_arg(stream)))

    def search_rows_sharded_device(self, row_ids, k: int, out_dist_ptr: int, out_rows_ptr: int, include_self: bool = False,
                                   stream: int | None = None) -> None:
        ids = self._row_ids(row_ids)
        check(self._h, self._lib.mi355dr_search_rows_sharded_device(
            self._h, ptr(ids, ctypes.c_int64), ids.shape[0], int(k), 1 if include_self else 0, ctypes.c_void_p(int(out_dist_ptr)),
            ctypes.c_void_p(int(out_rows_ptr)), _stream_arg(stream)))

    def search_range_rows_sharded_device(self, row_ids, radius, max_results: int, out_dist_ptr: int, out_rows_ptr: int,
                                         out_count_ptr: int, include_self: bool = False, stream: int | None = None) -> None:
        ids = self._row_ids(row_ids)
        r = self._radius(radius, ids.shape[0])
        check(self._h, self._lib.mi355dr_search_range_rows_sharded_device(
            self._h, ptr(ids, ctypes.c_int64), ids.shape[0], ptr(r, ctypes.c_double), int(max_results),
            1 if include_self else 0, ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)),
            ctypes.c_void_p(int(out_count_ptr)), _stream_arg(stream)))

    def search_mmr_sharded_device(self, q_ptr: int, B: int, k: int, fetch_k: int, out_dist_ptr: int, out_rows_ptr: int,
                                  lambda_mult: float = 0.5, stream: int | None = None) -> None:
        check(self._h, self._lib.mi355dr_search_mmr_sharded_device(
            self._h, ctypes.c_void_p(int(q_ptr)), int(B), int(k), int(fetch_k), float(lambda_mult),
            ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)), _stream_arg(stream)))

    def _device_results(self, B: int, width: int, with_count: bool, call):
        """Device buffers [B, width] float64 / int64 (and [B] int64) for one call of a _sharded_device form, downloaded."""
        dist = np.empty((B, width), dtype=np.float64)
        rows = np.empty((B, width), dtype=np.int64)
        count = np.empty(B, dtype=np.int64)
        bufs = [self.dev_alloc(max(dist.nbytes, 8)), self.dev_alloc(max(rows.nbytes, 8)), self.dev_alloc(max(count.nbytes, 8))]
        try:
            call(*bufs)
            if B and width:
                self.dev_download(bufs[0], dist)
                self.dev_download(bufs[1], rows)
            if B and with_count:
                self.dev_download(bufs[2], count)
        finally:
            for b in bufs:
                self.dev_free(b)
        return (dist, rows, count) if with_count else (dist, rows)

    def _device_queries(self, queries) -> tuple[np.ndarray, int]:
        q = self._queries_2d(queries)
        p = self.dev_alloc(max(q.nbytes, 8))
        if q.nbytes:
            self.dev_upload(p, q)
        return q, p

    def search_range_sharded(self, queries, radius, max_results: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`search_range` over the shards: the merged list and the summed count, the same on every rank."""
        q, qp = self._device_queries(queries)
        try:
            return self._device_results(q.shape[0], max(int(max_results), 0), True, lambda d, r, c: self.search_range_sharded_device(
                qp, q.shape[0], radius, max_results, d, r, c))
        finally:
            self.dev_free(qp)

    def search_mmr_sharded(self, queries, k: int, fetch_k: int, lambda_mult: float = 0.5) -> tuple[np.ndarray, np.ndarray]:
        """`search_mmr` over the shards: the sharded search at `fetch_k`, then the picks over the owners' staged vectors."""
        q, qp = self._device_queries(queries)
        try:
            return self._device_results(q.shape[0], max(int(k), 0), False, lambda d, r, _c: self.search_mmr_sharded_device(
                qp, q.shape[0], k, fetch_k, d, r, lambda_mult))
        finally:
            self.dev_free(qp)

    def search_rows_sharded(self, row_ids, k: int, include_self: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """`search_rows` over the shards: each id's vector comes from the rank that owns it."""
        ids = self._row_ids(row_ids)
        return self._device_results(ids.shape[0], max(int(k), 0), False, lambda d, r, _c: self.search_rows_sharded_device(
            ids, k, d, r, include_self))

    def search_range_rows_sharded(self, row_ids, radius, max_results: int,
                                  include_self: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`search_range_rows` over the shards."""
        ids = self._row_ids(row_ids)
        return self._device_results(ids.shape[0], max(int(max_results), 0), True,
                                    lambda d, r, c: self.search_range_rows_sharded_device(ids, radius, max_results, d, r, c, include_self))

    def mmr_select_sharded(self, queries, k: int, cand_rows, lambda_mult: float = 0.5) -> tuple[np.ndarray, np.ndarray]:
        """`mmr_select` over the shards: cand_rows [B, m] global rows, the same on every rank."""
        q = self._queries_2d(queries)
        ids = np.ascontiguousarray(cand_rows, dtype=np.int64)
        if ids.ndim == 1:
            ids = ids[None, :]
        if ids.ndim != 2 or ids.shape[0] != q.shape[0]:
            raise ValueError(f"cand_rows must be [B, m] with B = {q.shape[0]}, got {ids.shape}")
        B = q.shape[0]
        dist = np.empty((B, k), dtype=np.float64)
        rows = np.empty((B, k), dtype=np.int64)
        check(self._h, self._lib.mi355dr_mmr_select_sharded(self._h, ptr(q, ctypes.c_float), B, int(k), ptr(ids, ctypes.c_int64),
                                                            ids.shape[1], float(lambda_mult), ptr(dist, ctypes.c_double),
                                                            ptr(rows, ctypes.c_int64)))
        return dist, rows

    # ---- sparse store: tokenised documents, weighted / BM25 top-k (include/mi355dr.h "sparse store") ----
    @staticmethod
    def _ragged_i32(lists_or_flat, offsets, off_dtype) -> tuple[np.ndarray, np.ndarray]:
        """(flat int32, offsets [n + 1]) from a list of token lists (offsets None) or from the flat pair itself."""
        if offsets is None:
            lists = [np.asarray(t, dtype=np.int64).reshape(-1) for t in lists_or_flat]
            off = np.zeros(len(lists) + 1, dtype=np.int64)
            if lists:
                off[1:] = np.cumsum([t.shape[0] for t in lists])
            flat = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        else:
            flat = np.asarray(lists_or_flat, dtype=np.int64).reshape(-1)
            off = np.asarray(offsets, dtype=np.int64).reshape(-1)
            if off.shape[0] < 1 or off[0] != 0 or off[-1] != flat.shape[0] or np.any(np.diff(off) < 0):
                raise ValueError("offsets must start at 0, never decrease and end at the number of tokens")
        if flat.size and (flat.min() < np.iinfo(np.int32).min or flat.max() > np.iinfo(np.int32).max):
            raise ValueError("token ids must fit int32")
        if off[-1] > np.iinfo(off_dtype).max:
            raise ValueError("too many tokens for one call")
        return np.ascontiguousarray(flat, dtype=np.int32), np.ascontiguousarray(off, dtype=off_dtype)

    def add_sparse(self, token_lists, offsets=None) -> None:
        """Append tokenised documents: a list of int token lists, or (terms, offsets [n_docs + 1]).  A document without tokens
        takes an id and never matches.  A term id outside [0, 2^20) or a term more than 4095 times in one document: NativeError,
        nothing changes."""
        terms, off = self._ragged_i32(token_lists, offsets, np.int64)
        check(self._h, self._lib.mi355dr_add_sparse(self._h, ptr(terms, ctypes.c_int32), ptr(off, ctypes.c_int64), off.shape[0] - 1))

    @staticmethod
    def _sparse_ids(doc_ids) -> np.ndarray:
        ids = np.asarray(doc_ids)
        if ids.size and not np.issubdtype(ids.dtype, np.integer):
            raise ValueError("doc_ids must be integers")
        return np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)

    def set_sparse(self, doc_ids, token_lists, offsets=None) -> None:
        """Document doc_ids[j] becomes token_lists[j] (or terms[offsets[j]:offsets[j + 1]], the flat form of `add_sparse`): later
        searches, `sparse_df` and the stats answer as a fresh store given one `add_sparse` of the current documents.  No tokens
        removes the document (it keeps its id and never matches), tokens revive a removed one.  Ids are local (no `row_offset`).
        An id out of range or listed twice, a term id outside [0, 2^20), a term more than 4095 times in one document:
        NativeError, nothing changes."""
        ids = self._sparse_ids(doc_ids)
        terms, off = self._ragged_i32(token_lists, offsets, np.int64)
        if off.shape[0] - 1 != ids.shape[0]:
            raise ValueError(f"{ids.shape[0]} doc_ids for {off.shape[0] - 1} token lists")
        check(self._h, self._lib.mi355dr_set_sparse(self._h, ptr(ids, ctypes.c_int64), ptr(terms, ctypes.c_int32),
                                                    ptr(off, ctypes.c_int64), ids.shape[0]))

    def remove_sparse(self, doc_ids) -> None:
        """The documents lose their tokens: stored, holding their ids, never matching, no part of N, total_len or df.  Removing a
        document without tokens changes nothing."""
        ids = self._sparse_ids(doc_ids)
        check(self._h, self._lib.mi355dr_remove_sparse(self._h, ptr(ids, ctypes.c_int64), ids.shape[0]))

    def live_sparse(self) -> int:
        """Sparse documents with tokens: N of the statistics (`size_sparse` minus the documents without tokens)."""
        return int(self._lib.mi355dr_live_sparse(self._h))

    def size_sparse(self) -> int:
        """Stored sparse documents, with or without tokens."""
        return int(self._lib.mi355dr_size_sparse(self._h))

    def sparse_df(self, terms) -> np.ndarray:
        """Document frequency of each term (0 for unseen and out-of-range ids)."""
        t = np.ascontiguousarray(np.asarray(terms, dtype=np.int64).reshape(-1).clip(-1, 2**31 - 1), dtype=np.int32)
        out = np.zeros(t.shape[0], dtype=np.int64)
        check(self._h, self._lib.mi355dr_sparse_df(self._h, ptr(t, ctypes.c_int32), t.shape[0], ptr(out, ctypes.c_int64)))
        return out

    def _sparse_call(self, B: int, k: int, device_out: bool, host_call, device_call) -> tuple[np.ndarray, np.ndarray]:
        if device_out:  # the _device form into buffers of this call, downloaded
            return self._device_results(B, max(int(k), 0), False, lambda d, r, _c: check(self._h, device_call(
                ctypes.c_void_p(d), ctypes.c_void_p(r), _stream_arg(None))))
        dist = np.empty((B, max(int(k), 0)), dtype=np.float64)
        rows = np.empty((B, max(int(k), 0)), dtype=np.int64)
        check(self._h, host_call(ptr(dist, ctypes.c_double), ptr(rows, ctypes.c_int64)))
        return dist, rows

    def search_sparse(self, terms, weights, offsets, k: int, k1: float = 1.2, b: float = 0.75,
                      device_out: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """Weighted sparse top-k: query j is terms[offsets[j]:offsets[j + 1]] (distinct) with the weights alongside.  Returns
        (distance float64 [B, k] = -score, ids int64 [B, k]); NaN / -1 behind the matches."""
        t, off = self._ragged_i32(terms, offsets, np.int32)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != t.shape[0]:
            raise ValueError("weights must have one entry per term")
        B = off.shape[0] - 1
        a = (self._h, ptr(t, ctypes.c_int32), ptr(w, ctypes.c_double), ptr(off, ctypes.c_int32), B, int(k), float(k1), float(b))
        return self._sparse_call(B, k, device_out, lambda d, r: self._lib.mi355dr_search_sparse(*a, d, r),
                                 lambda d, r, s: self._lib.mi355dr_search_sparse_device(*a, d, r, s))

    def search_bm25(self, token_lists, k: int, k1: float = 1.2, b: float = 0.75, device_out: bool = False,
                    offsets=None) -> tuple[np.ndarray, np.ndarray]:
        """BM25 top-k of raw token queries (repeats count once, unseen terms are dropped; idf by libm's log on the host).
        Returns (distance float64 [B, k] = -score, ids int64 [B, k]).  `device_out`: through the _device form."""
        t, off = self._ragged_i32(token_lists, offsets, np.int32)
        B = off.shape[0] - 1
        a = (self._h, ptr(t, ctypes.c_int32), ptr(off, ctypes.c_int32), B, int(k), float(k1), float(b))
        return self._sparse_call(B, k, device_out, lambda d, r: self._lib.mi355dr_search_bm25(*a, d, r),
                                 lambda d, r, s: self._lib.mi355dr_search_bm25_device(*a, d, r, s))

    def search_bm25_device(self, token_lists, k: int, out_dist_ptr: int, out_ids_ptr: int, k1: float = 1.2, b: float = 0.75,
                           offsets=None, stream: int | None = None) -> None:
        """`search_bm25` into device buffers of the caller (float64 / int64 [B, k]); the queries stay on the host.  Complete
        on return."""
        t, off = self._ragged_i32(token_lists, offsets, np.int32)
        check(self._h, self._lib.mi355dr_search_bm25_device(
            self._h, ptr(t, ctypes.c_int32), ptr(off, ctypes.c_int32), off.shape[0] - 1, int(k), float(k1), float(b),
            ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_ids_ptr)), _stream_arg(stream)))

    # within a listed subset: a filter, not a view -- the statistics (N, avgdl, df) stay those of the whole store, so a listed
    # document's distance is bit for bit the unrestricted search's.  doc_ids are GLOBAL ids (local id + `row_offset`); ids
    # outside the store (negative ones and -1 padding included) are skipped
    def search_sparse_subset(self, terms, weights, offsets, k: int, doc_ids, k1: float = 1.2, b: float = 0.75,
                             device_out: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """`search_sparse` among the listed documents (one list for every query, duplicates count once, any order): the
        unrestricted ranking with the unlisted documents struck out, cut to k, NaN / -1 behind."""
        t, off = self._ragged_i32(terms, offsets, np.int32)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != t.shape[0]:
            raise ValueError("weights must have one entry per term")
        ids = self._sparse_ids(doc_ids)
        B = off.shape[0] - 1
        a = (self._h, ptr(t, ctypes.c_int32), ptr(w, ctypes.c_double), ptr(off, ctypes.c_int32), B, int(k), float(k1), float(b),
             ptr(ids, ctypes.c_int64), ids.shape[0])
        return self._sparse_call(B, k, device_out, lambda d, r: self._lib.mi355dr_search_sparse_subset(*a, d, r),
                                 lambda d, r, s: self._lib.mi355dr_search_sparse_subset_device(*a, d, r, s))

    def search_bm25_subset(self, token_lists, k: int, doc_ids, k1: float = 1.2, b: float = 0.75, device_out: bool = False,
                           offsets=None) -> tuple[np.ndarray, np.ndarray]:
        """`search_bm25` among the listed documents; the idf weights come from the WHOLE store's N and df."""
        t, off = self._ragged_i32(token_lists, offsets, np.int32)
        ids = self._sparse_ids(doc_ids)
        B = off.shape[0] - 1
        a = (self._h, ptr(t, ctypes.c_int32), ptr(off, ctypes.c_int32), B, int(k), float(k1), float(b), ptr(ids, ctypes.c_int64),
             ids.shape[0])
        return self._sparse_call(B, k, device_out, lambda d, r: self._lib.mi355dr_search_bm25_subset(*a, d, r),
                                 lambda d, r, s: self._lib.mi355dr_search_bm25_subset_device(*a, d, r, s))

    def _sparse_pool(self, doc_ids, B: int) -> np.ndarray:
        ids = np.asarray(doc_ids)
        if ids.size and not np.issubdtype(ids.dtype, np.integer):
            raise ValueError("doc_ids must be integers")
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if ids.ndim == 1 and B == 1:
            ids = ids[None, :]
        if ids.ndim != 2 or ids.shape[0] != B:
            raise ValueError(f"doc_ids must be [B, m] with B = {B}, got {ids.shape}")
        return ids

    def score_sparse_subset(self, terms, weights, offsets, doc_ids, k1: float = 1.2, b: float = 0.75) -> np.ndarray:
        """Exact distances (-score) of every query to ITS OWN candidates: doc_ids [B, m] -> float64 [B, m], NaN where the id is
        skipped or the document does not match the query; a duplicate is scored in every position."""
        t, off = self._ragged_i32(terms, offsets, np.int32)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != t.shape[0]:
            raise ValueError("weights must have one entry per term")
        B = off.shape[0] - 1
        ids = self._sparse_pool(doc_ids, B)
        out = np.empty(ids.shape, dtype=np.float64)
        check(self._h, self._lib.mi355dr_score_sparse_subset(self._h, ptr(t, ctypes.c_int32), ptr(w, ctypes.c_double),
                                                             ptr(off, ctypes.c_int32), B, float(k1), float(b),
                                                             ptr(ids, ctypes.c_int64), ids.shape[1], ptr(out, ctypes.c_double)))
        return out

    def score_bm25_subset(self, token_lists, doc_ids, k1: float = 1.2, b: float = 0.75, offsets=None) -> np.ndarray:
        """`score_sparse_subset` of raw token queries under the BM25 weights of the whole store."""
        t, off = self._ragged_i32(token_lists, offsets, np.int32)
        B = off.shape[0] - 1
        ids = self._sparse_pool(doc_ids, B)
        out = np.empty(ids.shape, dtype=np.float64)
        check(self._h, self._lib.mi355dr_score_bm25_subset(self._h, ptr(t, ctypes.c_int32), ptr(off, ctypes.c_int32), B, float(k1),
                                                           float(b), ptr(ids, ctypes.c_int64), ids.shape[1],
                                                           ptr(out, ctypes.c_double)))
        return out

    # over a row-sharded store (include/mi355dr.h "row-sharded sparse search"): this handle holds a contiguous run of the
    # documents with `row_offset` at its first one's global id, and a communicator.  Every rank passes the same arguments and
    # receives what ONE handle holding all shards' documents returns from the local method of the same name; N, avgdl and df
    # are gathered on every call.  The arguments are those of the local methods
    def _sparse_queries(self, bm25: bool, terms, weights, offsets) -> tuple[tuple, int, tuple]:
        """The query arguments of a weighted (terms, weights, offsets) or BM25 (token lists, offsets or None) call, B, and the
        arrays the pointers point into (the caller keeps them until the call has returned)."""
        t, off = self._ragged_i32(terms, offsets, np.int32)
        B = off.shape[0] - 1
        if bm25:
            return (ptr(t, ctypes.c_int32), ptr(off, ctypes.c_int32), B), B, (t, off)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != t.shape[0]:
            raise ValueError("weights must have one entry per term")
        return (ptr(t, ctypes.c_int32), ptr(w, ctypes.c_double), ptr(off, ctypes.c_int32), B), B, (t, w, off)

    def _sparse_sharded_device(self, name: str, bm25: bool, terms, weights, offsets, k: int, k1: float, b: float, doc_ids,
                               out_dist_ptr: int, out_ids_ptr: int, stream) -> None:
        q, _B, _keep = self._sparse_queries(bm25, terms, weights, offsets)
        tail = ()
        if doc_ids is not None:
            ids = self._sparse_ids(doc_ids)
            tail = (ptr(ids, ctypes.c_int64), ids.shape[0])
        check(self._h, getattr(self._lib, name)(self._h, *q, int(k), float(k1), float(b), *tail, ctypes.c_void_p(int(out_dist_ptr)),
                                                ctypes.c_void_p(int(out_ids_ptr)), _stream_arg(stream)))

    def search_sparse_sharded_device(self, terms, weights, offsets, k: int, out_dist_ptr: int, out_ids_ptr: int, k1: float = 1.2,
                                     b: float = 0.75, stream: int | None = None) -> None:
        """`search_sparse` over the shards into device buffers of the caller (float64 / int64 [B, k]); complete on return."""
        self._sparse_sharded_device("mi355dr_search_sparse_sharded_device", False, terms, weights, offsets, k, k1, b, None,
                                    out_dist_ptr, out_ids_ptr, stream)

    def search_bm25_sharded_device(self, token_lists, k: int, out_dist_ptr: int, out_ids_ptr: int, k1: float = 1.2,
                                   b: float = 0.75, offsets=None, stream: int | None = None) -> None:
        """`search_bm25_device` over the shards: the idf weights come from the N and df of ALL shards."""
        self._sparse_sharded_device("mi355dr_search_bm25_sharded_device", True, token_lists, None, offsets, k, k1, b, None,
                                    out_dist_ptr, out_ids_ptr, stream)

    def search_sparse_subset_sharded_device(self, terms, weights, offsets, k: int, doc_ids, out_dist_ptr: int, out_ids_ptr: int,
                                            k1: float = 1.2, b: float = 0.75, stream: int | None = None) -> None:
        """`search_sparse_subset` over the shards into device buffers; doc_ids are global ids, the same list on every rank."""
        self._sparse_sharded_device("mi355dr_search_sparse_subset_sharded_device", False, terms, weights, offsets, k, k1, b,
                                    doc_ids, out_dist_ptr, out_ids_ptr, stream)

    def search_bm25_subset_sharded_device(self, token_lists, k: int, doc_ids, out_dist_ptr: int, out_ids_ptr: int,
                                          k1: float = 1.2, b: float = 0.75, offsets=None, stream: int | None = None) -> None:
        """`search_bm25_subset` over the shards into device buffers."""
        self._sparse_sharded_device("mi355dr_search_bm25_subset_sharded_device", True, token_lists, None, offsets, k, k1, b,
                                    doc_ids, out_dist_ptr, out_ids_ptr, stream)

    def _sparse_sharded(self, device_method, B: int, k: int) -> tuple[np.ndarray, np.ndarray]:
        return self._device_results(B, max(int(k), 0), False, lambda d, r, _c: device_method(d, r))

    def search_sparse_sharded(self, terms, weights, offsets, k: int, k1: float = 1.2,
                              b: float = 0.75) -> tuple[np.ndarray, np.ndarray]:
        """`search_sparse` over the shards: (distance float64 [B, k], global ids int64 [B, k]), the same on every rank."""
        B = self._ragged_i32(terms, offsets, np.int32)[1].shape[0] - 1
        return self._sparse_sharded(lambda d, r: self.search_sparse_sharded_device(terms, weights, offsets, k, d, r, k1, b), B, k)

    def search_bm25_sharded(self, token_lists, k: int, k1: float = 1.2, b: float = 0.75,
                            offsets=None) -> tuple[np.ndarray, np.ndarray]:
        """`search_bm25` over the shards."""
        B = self._ragged_i32(token_lists, offsets, np.int32)[1].shape[0] - 1
        return self._sparse_sharded(lambda d, r: self.search_bm25_sharded_device(token_lists, k, d, r, k1, b, offsets), B, k)

    def search_sparse_subset_sharded(self, terms, weights, offsets, k: int, doc_ids, k1: float = 1.2,
                                     b: float = 0.75) -> tuple[np.ndarray, np.ndarray]:
        """`search_sparse_subset` over the shards."""
        B = self._ragged_i32(terms, offsets, np.int32)[1].shape[0] - 1
        return self._sparse_sharded(
            lambda d, r: self.search_sparse_subset_sharded_device(terms, weights, offsets, k, doc_ids, d, r, k1, b), B, k)

    def search_bm25_subset_sharded(self, token_lists, k: int, doc_ids, k1: float = 1.2, b: float = 0.75,
                                   offsets=None) -> tuple[np.ndarray, np.ndarray]:
        """`search_bm25_subset` over the shards."""
        B = self._ragged_i32(token_lists, offsets, np.int32)[1].shape[0] - 1
        return self._sparse_sharded(
            lambda d, r: self.search_bm25_subset_sharded_device(token_lists, k, doc_ids, d, r, k1, b, offsets), B, k)

    def _score_sharded(self, name: str, bm25: bool, terms, weights, offsets, doc_ids, k1: float, b: float) -> np.ndarray:
        q, B, _keep = self._sparse_queries(bm25, terms, weights, offsets)
        ids = self._sparse_pool(doc_ids, B)
        out = np.empty(ids.shape, dtype=np.float64)
        check(self._h, getattr(self._lib, name)(self._h, *q, float(k1), float(b), ptr(ids, ctypes.c_int64), ids.shape[1],
                                                ptr(out, ctypes.c_double)))
        return out

    def score_sparse_subset_sharded(self, terms, weights, offsets, doc_ids, k1: float = 1.2, b: float = 0.75) -> np.ndarray:
        """`score_sparse_subset` over the shards: each position holds its owner's value, NaN where no rank matches it."""
        return self._score_sharded("mi355dr_score_sparse_subset_sharded", False, terms, weights, offsets, doc_ids, k1, b)

    def score_bm25_subset_sharded(self, token_lists, doc_ids, k1: float = 1.2, b: float = 0.75, offsets=None) -> np.ndarray:
        """`score_bm25_subset` over the shards, under the BM25 weights of all shards' documents."""
        return self._score_sharded("mi355dr_score_bm25_subset_sharded", True, token_lists, None, offsets, doc_ids, k1, b)

    # ---- multi-vector ----
    def add_multivec(self, vecs, offsets) -> None:
        vecs = f32c(vecs)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if vecs.ndim != 2 or vecs.shape[1] != self.dim:
            raise ValueError(f"vecs must be [sum_T, {self.dim}]")
        if offsets.ndim != 1 or offsets.shape[0] < 1 or offsets[0] != 0 or offsets[-1] != vecs.shape[0]:
            raise ValueError("offsets must start at 0 and end at vecs.shape[0]")
        check(self._h, self._lib.mi355dr_add_multivec(self._h, ptr(vecs, ctypes.c_float),
                                                      ptr(offsets, ctypes.c_int64), offsets.shape[0] - 1))

    def add_multivec_device(self, vecs_ptr: int, offsets) -> None:
        """Docs whose token / patch vectors already sit in device memory ([sum_T, dim] fp32 at `vecs_ptr`, e.g. an
        encoder's output tensor): the padded store, its bf16 fragment copy and the screen's bound quantities are built
        by a kernel, nothing is copied to the host.  `offsets` is a host array [n_docs + 1]."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.ndim != 1 or offsets.shape[0] < 1 or offsets[0] != 0:
            raise ValueError("offsets must start at 0")
        check(self._h, self._lib.mi355dr_add_multivec_device(self._h, ctypes.c_void_p(int(vecs_ptr)),
                                                             ptr(offsets, ctypes.c_int64), offsets.shape[0] - 1))

    def n_docs(self) -> int:
        return int(self._lib.mi355dr_size_multivec(self._h))

    # ---- replace / remove documents in place (document ids are stable; include/mi355dr.h "update / remove in place (multi-vector)") ----
    @staticmethod
    def _doc_ids_offsets(doc_ids, offsets) -> tuple[np.ndarray, np.ndarray]:
        ids = np.ascontiguousarray(doc_ids, dtype=np.int64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if ids.ndim != 1 or offsets.ndim != 1 or offsets.shape[0] != ids.shape[0] + 1:
            raise ValueError("doc_ids must be [n] and offsets [n + 1]")
        return ids, offsets

    def set_multivec(self, doc_ids, vecs, offsets) -> None:
        """Document doc_ids[j] takes vecs[offsets[j]:offsets[j + 1]]: later searches see the store an `add_multivec` of the
        current contents would have built.  No vectors removes the document, vectors revive a removed one.  Ids out of range
        or repeated, decreasing offsets: NativeError (MI355DR_E_INVALID), nothing changes."""
        ids, offsets = self._doc_ids_offsets(doc_ids, offsets)
        vecs = f32c(vecs).reshape(-1, self.dim)
        if offsets[0] != 0 or offsets[-1] != vecs.shape[0]:
            raise ValueError("offsets must start at 0 and end at vecs.shape[0]")
        check(self._h, self._lib.mi355dr_set_multivec(self._h, ptr(ids, ctypes.c_int64), ptr(vecs, ctypes.c_float),
                                                      ptr(offsets, ctypes.c_int64), ids.shape[0]))

    def set_multivec_device(self, doc_ids, vecs_ptr: int, offsets) -> None:
        """The same with the new vectors ([offsets[-1], dim] fp32, contiguous) already on this device; ids and offsets stay
        on the host."""
        ids, offsets = self._doc_ids_offsets(doc_ids, offsets)
        check(self._h, self._lib.mi355dr_set_multivec_device(self._h, ptr(ids, ctypes.c_int64), ctypes.c_void_p(int(vecs_ptr)),
                                                             ptr(offsets, ctypes.c_int64), ids.shape[0]))

    def remove_multivec(self, doc_ids) -> None:
        """The documents lose their vectors: never returned again by any search; their ids (and every other document's) stay."""
        ids = np.ascontiguousarray(doc_ids, dtype=np.int64)
        self.set_multivec(ids, np.zeros((0, self.dim), np.float32), np.zeros(ids.shape[0] + 1, np.int64))

    def live_docs(self) -> int:
        """n_docs() minus the documents without vectors."""
        return int(self._lib.mi355dr_live_multivec(self._h))

    def search_maxsim(self, qtok, q_offsets, k: int) -> tuple[np.ndarray, np.ndarray]:
        """MaxSim top-k.  Returns (distance float32 [B,k] = -sum_i max_j <q_i,d_j>, doc rows int64 [B,k])."""
        qtok = f32c(qtok)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int32)
        B = q_offsets.shape[0] - 1
        dist = np.empty((B, k), dtype=np.float32)
        rows = np.empty((B, k), dtype=np.int64)
        check(self._h, self._lib.mi355dr_search_maxsim(self._h, ptr(qtok, ctypes.c_float),
                                                       ptr(q_offsets, ctypes.c_int32), B, int(k),
                                                       ptr(dist, ctypes.c_float), ptr(rows, ctypes.c_int64)))
        return dist, rows

    def search_maxsim_device(self, qtok_ptr: int, q_offsets, k: int, out_dist_ptr: int, out_rows_ptr: int,
                             stream: int | None = None) -> None:
        """MaxSim top-k with the query vectors ([sum_nq, dim] fp32 at `qtok_ptr`) and the results (fp32 [B,k] at
        `out_dist_ptr`, int64 [B,k] at `out_rows_ptr`) in device memory; `q_offsets` is a host array [B+1]."""
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int32)
        check(self._h, self._lib.mi355dr_search_maxsim_device(
            self._h, ctypes.c_void_p(int(qtok_ptr)), ptr(q_offsets, ctypes.c_int32), q_offsets.shape[0] - 1, int(k),
            ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)),
            _stream_arg(stream)))

    # ---- MaxSim search within a listed subset of documents (include/mi355dr.h) ----
    def search_maxsim_subset(self, qtok, q_offsets, k: int, doc_ids) -> tuple[np.ndarray, np.ndarray]:
        """MaxSim top-k among the listed documents only: `search_maxsim` with `AND id = ANY(doc_ids)`.  doc_ids: global ids
        as the searches return them, ONE list for all queries, in any order; ids outside the index (-1 padding included) and
        documents without vectors are skipped, an id listed twice counts once.  Same fp32 distances, order (distance, then
        document) and NaN / -1 tail as `search_maxsim`; equal to `view(doc_ids=...).search_maxsim(...)` without building the
        view.  Returns (distance float32 [B,k], docs int64 [B,k])."""
        qtok = f32c(qtok).reshape(-1, self.dim)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int32)
        ids = self._row_ids(doc_ids)
        B = q_offsets.shape[0] - 1
        dist = np.empty((B, k), dtype=np.float32)
        docs = np.empty((B, k), dtype=np.int64)
        check(self._h, self._lib.mi355dr_search_maxsim_subset(
            self._h, ptr(qtok, ctypes.c_float), ptr(q_offsets, ctypes.c_int32), B, int(k), ptr(ids, ctypes.c_int64),
            ids.shape[0], ptr(dist, ctypes.c_float), ptr(docs, ctypes.c_int64)))
        return dist, docs

    def search_maxsim_subset_device(self, qtok_ptr: int, q_offsets, k: int, doc_ids, out_dist_ptr: int, out_rows_ptr: int,
                                    stream: int | None = None) -> None:
        """The same with the query vectors and the results in device memory (the layout of `search_maxsim_device`);
        `q_offsets` and `doc_ids` stay on the host.  Complete on return."""
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int32)
        ids = self._row_ids(doc_ids)
        check(self._h, self._lib.mi355dr_search_maxsim_subset_device(
            self._h, ctypes.c_void_p(int(qtok_ptr)), ptr(q_offsets, ctypes.c_int32), q_offsets.shape[0] - 1, int(k),
            ptr(ids, ctypes.c_int64), ids.shape[0], ctypes.c_void_p(int(out_dist_ptr)), ctypes.c_void_p(int(out_rows_ptr)),
            _stream_arg(stream)))

    def maxsim_subset(self, qtok, q_offsets, doc_ids, clamp0: bool = False) -> np.ndarray:
        """Exact MaxSim distance of each query to its own list of docs: doc_ids [B, m] -> distances [B, m] (NaN = skipped).
        `clamp0`: every query vector contributes max(0, max_j <q_i, d_j>) (the ColBERT reranker's MaxSim)."""
        qtok = f32c(qtok).reshape(-1, self.dim)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int32)
        ids = np.ascontiguousarray(doc_ids, dtype=np.int64)
        B = q_offsets.shape[0] - 1
        if ids.ndim != 2 or ids.shape[0] != B:
            raise ValueError("doc_ids must be [B, m]")
        out = np.empty(ids.shape, dtype=np.float32)
        check(self._h, self._lib.mi355dr_maxsim_subset_ex(self._h, ptr(qtok, ctypes.c_float), ptr(q_offsets, ctypes.c_int32),
                                                          B, ptr(ids, ctypes.c_int64), ids.shape[1], 1 if clamp0 else 0,
                                                          ptr(out, ctypes.c_float)))
        return out

    # ---- MaxSim explained: the terms of the sum (include/mi355dr.h) ----
    def multivec_token_counts(self, doc_ids) -> np.ndarray:
        """Token vectors of the listed GLOBAL documents: int32 [n]; 0 = a document without vectors, -1 = not in this index."""
        ids = np.ascontiguousarray(doc_ids, dtype=np.int64).reshape(-1)
        out = np.empty(ids.shape[0], dtype=np.int32)
        check(self._h, self._lib.mi355dr_multivec_token_counts(self._h, ptr(ids, ctypes.c_int64), ids.shape[0],
                                                               ptr(out, ctypes.c_int32)))
        return out

    def maxsim_align(self, qtok, q_offsets, doc_ids, clamp0: bool = False, want_dist: bool = True) -> MaxSimAlignment:
        """Token alignment of each query with its own list of docs (doc_ids [B, m], the shapes of `maxsim_subset`): for every
        query vector the best dot over the document's tokens and the lowest token index that reaches it.  `dist` is bit for
        bit `maxsim_subset(qtok, q_offsets, doc_ids, clamp0)`."""
        qtok = f32c(qtok).reshape(-1, self.dim)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int32)
        ids = np.ascontiguousarray(doc_ids, dtype=np.int64)
        B = q_offsets.shape[0] - 1
        if ids.ndim != 2 or ids.shape[0] != B:
            raise ValueError("doc_ids must be [B, m]")
        V, m = int(q_offsets[B] - q_offsets[0]) if B > 0 else 0, ids.shape[1]
        values = np.empty((V, m), dtype=np.float32)
        tokens = np.empty((V, m), dtype=np.int32)
        dist = np.empty((B, m), dtype=np.float32) if want_dist else None
        check(self._h, self._lib.mi355dr_maxsim_align(
            self._h, ptr(qtok, ctypes.c_float), ptr(q_offsets, ctypes.c_int32), B, ptr(ids, ctypes.c_int64), m,
            1 if clamp0 else 0, ptr(values, ctypes.c_float), ptr(tokens, ctypes.c_int32),
            ptr(dist, ctypes.c_float) if want_dist else None))
        return MaxSimAlignment(values, tokens, dist)

    def maxsim_map(self, qtok, q_offsets, pair_query, pair_doc) -> list[np.ndarray]:
        """Similarity maps of the listed (query, GLOBAL document) pairs: one float32 [nq_p, T_p] array per pair, element
        [i, j] = <q_i, d_j>; T_p = 0 for a document without vectors or outside this index."""
        qtok = f32c(qtok).reshape(-1, self.dim)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int32)
        pq = np.ascontiguousarray(pair_query, dtype=np.int32).reshape(-1)
        pd = np.ascontiguousarray(pair_doc, dtype=np.int64).reshape(-1)
        B, P = q_offsets.shape[0] - 1, pq.shape[0]
        if pd.shape[0] != P:
            raise ValueError("pair_query and pair_doc must have one entry per pair")
        if P and (pq.min() < 0 or pq.max() >= B):
            raise ValueError("pair_query out of range")
        T = np.maximum(self.multivec_token_counts(pd), 0).astype(np.int64)
        nq = (q_offsets[1:] - q_offsets[:-1]).astype(np.int64)[pq] if P else np.zeros(0, np.int64)
        off = np.zeros(P + 1, dtype=np.int64)
        np.cumsum(nq * T, out=off[1:])
        out = np.empty(max(int(off[P]), 1), dtype=np.float32)
        check(self._h, self._lib.mi355dr_maxsim_map(
            self._h, ptr(qtok, ctypes.c_float), ptr(q_offsets, ctypes.c_int32), B, ptr(pq, ctypes.c_int32),
            ptr(pd, ctypes.c_int64), P, ptr(off, ctypes.c_int64), ptr(out, ctypes.c_float)))
        return [out[off[p]:off[p + 1]].reshape(int(nq[p]), int(T[p])).copy() for p in range(P)]

    # ---- Guided Query Refinement of candidate pools (reference gqr_hybrid.py:306-362) ----
    @staticmethod
    def _gqr_pool(pool, comp) -> tuple[np.ndarray, np.ndarray]:
        pool = np.ascontiguousarray(pool, dtype=np.int64)
        comp = np.ascontiguousarray(comp, dtype=np.float64)
        if pool.ndim != 2 or comp.shape != pool.shape:
            raise ValueError("candidate pool and complementary distribution must both be [B, P]")
        return pool, comp

    def gqr_refine(self, queries, cand_rows, comp_dist, n_steps: int, learning_rate: float, temperature: float,
                   mixture_alpha: float) -> np.ndarray:
        """Refine each query embedding against its candidate rows; returns the refined cosine scores float64 [B, P]
        (NaN at the -1 padding of a pool)."""
        pool, comp = self._gqr_pool(cand_rows, comp_dist)
        q = np.ascontiguousarray(queries, dtype=np.float64).reshape(pool.shape[0], self.dim)
        out = np.empty(pool.shape, dtype=np.float64)
        check(self._h, self._lib.mi355dr_gqr_refine(
            self._h, ptr(q, ctypes.c_double), pool.shape[0], ptr(pool, ctypes.c_int64), pool.shape[1],
            ptr(comp, ctypes.c_double), int(n_steps), float(learning_rate), float(temperature), float(mixture_alpha),
            ptr(out, ctypes.c_double)))
        return out

    def gqr_refine_maxsim(self, qtok, q_offsets, doc_ids, comp_dist, n_steps: int, learning_rate: float,
                          temperature: float, mixture_alpha: float) -> np.ndarray:
        """Multi-vector form: refine each query matrix against its candidate docs; refined mean-of-max scores [B, P]."""
        pool, comp = self._gqr_pool(doc_ids, comp_dist)
        q = np.ascontiguousarray(qtok, dtype=np.float64).reshape(-1, self.dim)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int32)
        if q_offsets.shape[0] != pool.shape[0] + 1 or int(q_offsets[-1]) != q.shape[0]:
            raise ValueError("q_offsets must be [B+1] and end at the number of query vectors")
        out = np.empty(pool.shape, dtype=np.float64)
        check(self._h, self._lib.mi355dr_gqr_refine_maxsim(
            self._h, ptr(q, ctypes.c_double), ptr(q_offsets, ctypes.c_int32), pool.shape[0], ptr(pool, ctypes.c_int64),
            pool.shape[1], ptr(comp, ctypes.c_double), int(n_steps), float(learning_rate), float(temperature),
            float(mixture_alpha), ptr(out, ctypes.c_double)))
        return out

    def gqr_refine_scores(self, primary_scores, counts, comp_dist, n_steps: int, learning_rate: float,
                          temperature: float, mixture_alpha: float) -> np.ndarray:
        """Score-space form (no vectors): the primary scores themselves are refined; [B, P], counts[b] live entries."""
        z = np.ascontiguousarray(primary_scores, dtype=np.float64)
        comp = np.ascontiguousarray(comp_dist, dtype=np.float64)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        if z.ndim != 2 or comp.shape != z.shape or counts.shape != (z.shape[0],):
            raise ValueError("primary_scores / comp_dist must be [B, P] and counts [B]")
        out = np.empty(z.shape, dtype=np.float64)
        check(self._h, self._lib.mi355dr_gqr_refine_scores(
            self._h, ptr(z, ctypes.c_double), ptr(counts, ctypes.c_int32), z.shape[0], z.shape[1],
            ptr(comp, ctypes.c_double), int(n_steps), float(learning_rate), float(temperature), float(mixture_alpha),
            ptr(out, ctypes.c_double)))
        return out

    # ---- options / stats / timing ----
    def set_option(self, key: str, value: int | str) -> None:
        if key == "path" and isinstance(value, str):
            value = PATHS[value]
        if key == "screen_dtype" and isinstance(value, str):
            value = SCREEN_DTYPES[value]
        check(self._h, self._lib.mi355dr_set_option(self._h, key.encode(), int(value)))

    def stat(self, key: str) -> int:
        out = ctypes.c_int64(0)
        check(self._h, self._lib.mi355dr_get_stat(self._h, key.encode(), ctypes.byref(out)))
        return int(out.value)

    def reset_stats(self) -> None:
        check(self._h, self._lib.mi355dr_reset_stats(self._h))

    def timer_start(self) -> None:
        check(self._h, self._lib.mi355dr_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = ctypes.c_double(0.0)
        check(self._h, self._lib.mi355dr_timer_stop(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def synchronize(self) -> None:
        check(self._h, self._lib.mi355dr_synchronize(self._h))

    # ---- raw device buffers (tests / bench without torch) ----
    def dev_alloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        check(self._h, self._lib.mi355dr_dev_alloc(self._h, int(nbytes), ctypes.byref(p)))
        return int(p.value)

    def dev_free(self, p: int) -> None:
        check(self._h, self._lib.mi355dr_dev_free(self._h, ctypes.c_void_p(int(p))))

    def dev_upload(self, dst: int, arr: np.ndarray) -> None:
        arr = np.ascontiguousarray(arr)
        check(self._h, self._lib.mi355dr_dev_upload(self._h, ctypes.c_void_p(int(dst)),
                                                    ctypes.c_void_p(arr.ctypes.data), arr.nbytes))

    def dev_download(self, src: int, arr: np.ndarray) -> None:
        assert arr.flags["C_CONTIGUOUS"]
        check(self._h, self._lib.mi355dr_dev_download(self._h, ctypes.c_void_p(arr.ctypes.data),
                                                      ctypes.c_void_p(int(src)), arr.nbytes))

    # ---- test hooks ----
    def debug_screen_dense(self, queries, row0: int, n: int) -> np.ndarray:
        q = f32c(queries)
        out = np.empty((q.shape[0], n), dtype=np.float32)
        check(self._h, self._lib.mi355dr_debug_screen_dense(self._h, ptr(q, ctypes.c_float), q.shape[0], int(row0),
                                                            int(n), ptr(out, ctypes.c_float)))
        return out

    def debug_screen_hits(self, queries, row0: int, n: int, thr, cap: int = 2048) -> dict:
        """One production screen launch over rows [row0, row0 + n) with the caller's thresholds (mi355dr_debug_screen_hits).
        Returns {"kernel": 0 k_screen / 1 k_screen_stream / 2 k_screen256c / 3 k_screen_rq, "count" [B]: the device's
        counters (may exceed cap), "status" [B], and the lists' entries flat, in list order: "q", "row", "val"} -- without
        the entries of rows outside the int8 shadow (their value is a stale accumulator's); "dropped" [B] counts those."""
        q = f32c(queries)
        B = q.shape[0]
        t = f32c(thr)
        if t.shape != (B,):
            raise ValueError("thr must hold one threshold per query")
        count = np.empty(B, dtype=np.int32)
        status = np.empty(B, dtype=np.int32)
        rows = np.empty((B, cap), dtype=np.int32)
        vals = np.empty((B, cap), dtype=np.float32)
        kernel = ctypes.c_int(-1)
        check(self._h, self._lib.mi355dr_debug_screen_hits(self._h, ptr(q, ctypes.c_float), B, int(row0), int(n),
                                                           ptr(t, ctypes.c_float), int(cap), ptr(count, ctypes.c_int),
                                                           ptr(rows, ctypes.c_int32), ptr(vals, ctypes.c_float),
                                                           ptr(status, ctypes.c_int), ctypes.byref(kernel)))
        held = np.arange(cap)[None, :] < np.minimum(count, cap)[:, None]
        flagged = held & (rows < 0)
        keep = held & ~flagged
        return {"kernel": int(kernel.value), "count": count, "status": status, "dropped": flagged.sum(axis=1),
                "q": np.nonzero(keep)[0].astype(np.int32), "row": rows[keep], "val": vals[keep]}

    MS_FORMS = ("none", "generic", "d128", "d128_packed", "wg", "wg_packed", "list_generic", "list_d128")

    def debug_maxsim_pass(self, qtok, q_offsets, k: int, doc_ids=None, list_cap: int = 8192) -> dict:
        """ONE pass of `search_maxsim` (with `doc_ids`: of `search_maxsim_subset`) through the search's own functions, and what it
        computed (mi355dr_debug_maxsim_pass).  Returns {"live" [B]: row of each query in the pass or -1, "screen" [n_live, n_docs]:
        the screen distances as the kernel left them over rows poisoned with 0xFFFFFFFF, "two_e" [n_live], "form": {"family"
        (MS_FORMS), "ncb", "waves", "bps", "pipe", "now", "grid"}, "cand_cap", "tighten_max", and for k <= 64 on a screened pass
        "lists": {"wide" / "starter" / "final": per live query {"ids" (the entries held), "count", "overflow"}; wide also "sd"}
        (else None)}.  NativeError (MI355DR_E_INVALID) when the queries are not one pass; the index stays usable."""
        qtok = f32c(qtok).reshape(-1, self.dim)
        q_offsets = np.ascontiguousarray(q_offsets, dtype=np.int32)
        B = q_offsets.shape[0] - 1
        ids = None if doc_ids is None else self._row_ids(doc_ids)
        n_docs = self.n_docs()
        live = np.full(max(B, 1), -1, dtype=np.int32)
        screen = np.empty((max(B, 1), max(n_docs, 1)), dtype=np.float32)
        two_e = np.empty(max(B, 1), dtype=np.float32)
        lists = np.full((3, max(B, 1), list_cap), -1, dtype=np.int32)
        ctl = np.zeros((3, max(B, 1), 2), dtype=np.int32)
        sd = np.full((max(B, 1), list_cap), np.nan, dtype=np.float32)
        form = np.zeros(8, dtype=np.int32)
        info = np.zeros(4, dtype=np.int32)
        check(self._h, self._lib.mi355dr_debug_maxsim_pass(
            self._h, ptr(qtok, ctypes.c_float), ptr(q_offsets, ctypes.c_int32), B, int(k),
            None if ids is None else ptr(ids, ctypes.c_int64), 0 if ids is None else ids.shape[0], int(list_cap),
            ptr(live, ctypes.c_int), ptr(screen, ctypes.c_float), ptr(two_e, ctypes.c_float), ptr(lists, ctypes.c_int32),
            ptr(ctl, ctypes.c_int), ptr(sd, ctypes.c_float), ptr(form, ctypes.c_int), ptr(info, ctypes.c_int)))
        n_live, cap = int(info[0]), int(info[1])
        out = {"live": live[:B], "two_e": two_e[:n_live],
               "screen": screen.reshape(-1)[:n_live * n_docs].reshape(n_live, n_docs),
               "form": {"family": self.MS_FORMS[int(form[0])], "ncb": int(form[1]), "waves": int(form[2]), "bps": int(form[3]),
                        "pipe": int(form[4]), "now": int(form[5]), "grid": int(form[6])},
               "cand_cap": cap, "tighten_max": int(info[3]), "lists": None}
        if info[2]:
            out["lists"] = {}
            for sec, name in enumerate(("wide", "starter", "final")):
                rows = []
                for r in range(n_live):
                    held = min(int(ctl[sec, r, 0]), cap, list_cap)
                    e = {"ids": lists[sec, r, :held].copy(), "count": int(ctl[sec, r, 0]), "overflow": int(ctl[sec, r, 1])}
                    if sec == 0:
                        e["sd"] = sd[r, :held].copy()
                    rows.append(e)
                out["lists"][name] = rows
        return out

    def debug_i8_state(self, queries, g0: int, n_groups: int) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """int8 screen: (S_q [B], kq [B], S_g [n_groups], e_g [n_groups]) -- screen value = S_q S_g (q8.c8) + e_g kq."""
        q = f32c(queries)
        sq = np.empty(q.shape[0], dtype=np.float32)
        kq = np.empty(q.shape[0], dtype=np.float32)
        st = np.empty(n_groups, dtype=np.float32)
        er = np.empty(n_groups, dtype=np.float32)
        check(self._h, self._lib.mi355dr_debug_i8_state(self._h, ptr(q, ctypes.c_float), q.shape[0], ptr(sq, ctypes.c_float),
                                                        ptr(kq, ctypes.c_float), int(g0), int(n_groups),
                                                        ptr(st, ctypes.c_float), ptr(er, ctypes.c_float)))
        return sq, kq, st, er

    def debug_screen_bound(self, queries) -> np.ndarray:
        """Per-query bound E of the active screen dtype: exact cosine <= screen value + E."""
        q = f32c(queries)
        out = np.empty(q.shape[0], dtype=np.float32)
        check(self._h, self._lib.mi355dr_debug_screen_bound(self._h, ptr(q, ctypes.c_float), q.shape[0],
                                                            ptr(out, ctypes.c_float)))
        return out

    def debug_spec_model(self, queries, k: int) -> dict:
        """The head of a speculative pass at `k` (mi355dr_debug_spec_model): {"moments" [B, slabs, 2]: per-slab sum and sum of
        squares of the sample's screen estimates, "thr_rigorous" [B], "thr_used" [B], "zq", "sample_rows", "i8"}.
        NativeError (MI355DR_E_UNSUPPORTED) where a first attempt at `k` would not speculate."""
        q = f32c(queries)
        B = q.shape[0]
        moments = np.empty((B, 256, 2), dtype=np.float32)
        rigorous = np.empty(B, dtype=np.float32)
        used = np.empty(B, dtype=np.float32)
        zq = ctypes.c_double(0.0)
        rows = ctypes.c_int64(0)
        slabs = ctypes.c_int(0)
        i8 = ctypes.c_int(0)
        check(self._h, self._lib.mi355dr_debug_spec_model(self._h, ptr(q, ctypes.c_float), B, int(k), ptr(moments, ctypes.c_float),
                                                          ptr(rigorous, ctypes.c_float), ptr(used, ctypes.c_float),
                                                          ctypes.byref(zq), ctypes.byref(rows), ctypes.byref(slabs),
                                                          ctypes.byref(i8)))
        n = int(slabs.value)
        return {"moments": moments.reshape(-1)[:B * n * 2].reshape(B, n, 2).copy(), "thr_rigorous": rigorous, "thr_used": used,
                "zq": float(zq.value), "sample_rows": int(rows.value), "i8": bool(i8.value)}

    def debug_rescore(self, queries, pair_q, pair_row) -> tuple[np.ndarray, np.ndarray]:
        q = f32c(queries)
        pq = np.ascontiguousarray(pair_q, dtype=np.int32)
        pr = np.ascontiguousarray(pair_row, dtype=np.int64)
        dot = np.empty(pq.shape[0], dtype=np.float32)
        dist = np.empty(pq.shape[0], dtype=np.float64)
        check(self._h, self._lib.mi355dr_debug_rescore(self._h, ptr(q, ctypes.c_float), q.shape[0],
                                                       ptr(pq, ctypes.c_int32), ptr(pr, ctypes.c_int64), pq.shape[0],
                                                       ptr(dot, ctypes.c_float), ptr(dist, ctypes.c_double)))
        return dot, dist
