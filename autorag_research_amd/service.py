"""Mi355RetrievalService -- host-side mirror of RetrievalPipelineService for the Vector Search path.

Same method names, argument meaning, return shapes and error behaviour as the reference
(autorag_research/orm/service/retrieval_pipeline.py):
  vector_search(query_ids, top_k, search_mode)          :467-525  score = 1 - distance | -distance / n_q
  vector_search_by_embedding(embedding, top_k)          :527-550
  run_pipeline / run_image_pipeline / _run_pipeline     :184-357  paging, resume-skip, retry, persistence, stats
  _collect_retrieval_results                            :151-182
  _make_retrieval_result                                :374-384  {"doc_id","score","content"}
  find_query_by_text                                    :386-400
The difference is WHERE the arithmetic runs: the two SQL operators the reference sends to PostgreSQL
(orm/repository/base.py:409-415 `<=>`, :518-524 `@#`) are answered by libmi355dr on the GPU, and a whole
list of query ids is scored as ONE block per corpus pass instead of one SQL statement per query.
"""

from __future__ import annotations

import asyncio
import logging
import os
from collections.abc import Awaitable, Callable
from typing import Any, Literal, NamedTuple

import numpy as np

from .index import Mi355Index
from .store import ChunkTable, InMemoryStore, UowStore

logger = logging.getLogger("AutoRAG-Research")

RetrievalFunc = Callable[[int | str, int], Awaitable[list[dict[str, Any]]]]


class _World:
    """The process group a pipeline runs in when it is launched one process per GPU (`torchrun --nproc-per-node N`, or any
    launcher that initialises torch.distributed before the Executor constructs its pipelines): every rank constructs the same
    pipeline over the same database; the corpus is ROW-SHARDED over the ranks (multi-vector tables by cumulative token
    count), every page of `run()` is answered by all ranks together -- local top-k, one all-gather over RCCL / xGMI, merge --
    and rank 0 alone reads the page's query ids and writes the results (reference caller: executor.py:383-463 ->
    pipelines/retrieval/base.py:156-199 -> retrieval_pipeline.py:184-307)."""

    def __init__(self, dist: Any):
        self.dist = dist
        self.rank, self.size = dist.get_rank(), dist.get_world_size()
        # The plugin's own collectives can be given a deadline: MI355DR_COLLECTIVE_TIMEOUT_S = seconds makes every rank create
        # (together: `new_group` is itself a collective, and `detect()` runs on every rank when the pipeline is constructed) a
        # group over the whole world with that timeout, and every collective below -- and the sharded searchers' -- uses it.
        # A rank that died or left through a rank-local error while its peers are inside a collective then costs them that many
        # seconds and a RuntimeError instead of the launcher's default (30 min under gloo, 10 under nccl) -- `agree` reconciles
        # failures OUTSIDE collectives only.  Unset / 0: the default group, as before.
        self.group = None
        try:
            t = float(os.environ.get("MI355DR_COLLECTIVE_TIMEOUT_S", "0") or 0)
        except ValueError:
            t = 0.0
        if t > 0:
            import datetime  # noqa: PLC0415

            self.group = dist.new_group(ranks=list(range(self.size)), timeout=datetime.timedelta(seconds=t))

    @classmethod
    def detect(cls) -> "_World | None":
        if os.environ.get("MI355DR_DISTRIBUTED", "1") == "0":
            return None
        try:
            import torch.distributed as dist  # noqa: PLC0415
        except ImportError:  # pragma: no cover
            return None
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() < 2:
            return None
        return cls(dist)

    def from_root(self, make: Callable[[], Any]) -> Any:
        """`make()` on rank 0, its (picklable) value on every rank.  An exception raised by `make()` on rank 0 travels the
        same way and is re-raised on EVERY rank: rank 0 always reaches the broadcast, so the other ranks never block on a
        collective that rank 0 left through an exception (a database error in `get_or_create_pipeline` / `next_page`)."""
        outcome = None
        if self.rank == 0:
            try:
                outcome = (True, make())
            except Exception as e:  # noqa: BLE001 - re-raised by share_outcome, on every rank
                outcome = (False, self._portable(e))
        return self.share_outcome(outcome)

    def share_outcome(self, outcome: tuple[bool, Any] | None) -> Any:
        """Rank 0's `(True, value)` or `(False, portable exception)` on every rank: the value returned, the exception raised."""
        box: list[Any] = [outcome]
        self.dist.broadcast_object_list(box, src=0, group=self.group)
        ok, value = box[0]
        if not ok:
            raise value
        return value

    @staticmethod
    def _portable(e: Exception) -> Exception:
        """The exception itself when it pickles (ValueError, KeyError ... the ones the reference's callers test for), else a
        RuntimeError carrying its text."""
        import pickle  # noqa: PLC0415

        try:
            pickle.loads(pickle.dumps(e))
        except Exception:  # noqa: BLE001
            return RuntimeError(f"{type(e).__name__}: {e}")
        return e

    def agree(self, ok: bool) -> bool:
        """True iff `ok` on every rank: ranks settle the outcome of a rank-local step BEFORE any of them branches into a
        different sequence of collectives (block answer vs per-query fallback vs retry)."""
        flags: list[Any] = [None] * self.size
        self.dist.all_gather_object(flags, bool(ok), group=self.group)
        return all(flags)

    def same_everywhere(self, what: str, digest: str) -> None:
        """Fail loudly, on every rank, when the ranks did not compute the same `digest` (the exported table's key order:
        global row ids are positions in that order, so two ranks that saw different orders would silently map each other's
        rows to the wrong primary keys)."""
        seen: list[Any] = [None] * self.size
        self.dist.all_gather_object(seen, digest, group=self.group)
        if any(d != seen[0] for d in seen):
            raise RuntimeError(f"{what}: the ranks exported different tables ({len(set(seen))} distinct digests over "
                               f"{self.size} ranks) -- the table changed during the export or the keys are not totally "
                               "ordered; refusing to search with inconsistent global row ids")

    def bind_device(self, device: int) -> None:
        """nccl collectives and broadcast_object_list run on torch's CURRENT device: make it this rank's GPU (a launcher
        that did not call torch.cuda.set_device would run every rank's collectives on cuda:0 -- a duplicate-GPU error or a
        hang).  No-op on the gloo backend."""
        if self.dist.get_backend() != "nccl":
            return
        import torch  # noqa: PLC0415

        torch.cuda.set_device(device)


def _table_digest(table: ChunkTable) -> str:
    """Key order + NULL pattern of an exported table (what global row ids depend on)."""
    import hashlib  # noqa: PLC0415

    h = hashlib.sha256()
    h.update(repr(len(table.ids)).encode())
    for pk in table.ids:
        h.update(repr(pk).encode())
        h.update(b"\x00")
    if table.embedding is not None:
        h.update(np.ascontiguousarray(np.isnan(table.embedding).all(axis=1)).tobytes())
    if table.mv_offsets is not None:
        h.update(np.ascontiguousarray(table.mv_offsets, dtype=np.int64).tobytes())
    return h.hexdigest()


class _SinglePlan(NamedTuple):  # what a newer export asks of the single-vector index (_UnitIndex._single_difference)
    emb: np.ndarray         # the new column, float32
    null: np.ndarray        # [n_new] bool: NULL in the new export
    was_null: np.ndarray    # [n_old] bool: NULL in the old one
    update: np.ndarray      # [n_old] bool: holds a vector now that differs from the old one (a revived NULL included)
    remove: np.ndarray      # [n_old] bool: became NULL


class _MultiPlan(NamedTuple):   # ... and of the multi-vector store (_UnitIndex._multi_difference)
    off: np.ndarray         # the new offsets, int64
    tok: np.ndarray         # the new token rows, float32
    changed: np.ndarray     # positions < n_old whose documents differ


class _DevScratch:
    """Named device buffers of a unit that grow and are reused page after page (raw hipMalloc blocks: any open handle of
    the device allocates and frees them)."""

    def __init__(self) -> None:
        self._bufs: dict[str, tuple[int, int]] = {}

    def take(self, ix: Mi355Index, name: str, nbytes: int) -> int:
        ptr, have = self._bufs.get(name, (0, 0))
        if have < nbytes:
            if ptr:
                ix.dev_free(ptr)
            self._bufs.pop(name, None)
            ptr = ix.dev_alloc(nbytes)
            self._bufs[name] = (ptr, nbytes)
        return ptr

    def drop(self, ix: Mi355Index, name: str) -> None:
        ptr, _ = self._bufs.pop(name, (0, 0))
        if ptr:
            ix.dev_free(ptr)

    def release(self, ix: Mi355Index | None) -> None:
        if ix is not None:
            for name in list(self._bufs):
                self.drop(ix, name)
        self._bufs.clear()

    def holds(self, name: str, ptr: int) -> bool:
        """`name` is still the block at `ptr` (it has not been dropped, released or regrown since)."""
        return bool(ptr) and self._bufs.get(name, (0, 0))[0] == ptr


# The default depth of a `per_source` search over a leg that cannot deepen (`within`, MaxSim, BM25), as a multiple of top_k.
# Not measured for these legs: 4 is the depth at which the search form needed the fewest extra rounds on sources of 8
# near-copies, taken over as a starting point.  A caller who knows its sources passes source_fetch_k.
LIST_SOURCE_FETCH_MULT = 4


def source_key_table(ids: list, source_of: Any, pos_of_row: np.ndarray | None = None) -> np.ndarray:
    """The key table of a `per_source` search (include/mi355dr.h "source-capped lists and search") in the id space of one leg:
    int64, entry j = the source of the chunk the leg returns as id j, -1 where it has none.  `source_of`: primary key -> source
    (any hashable; a missing key or None = no source, never capped); the sources are numbered in first-seen table order.
    `pos_of_row`: the leg's id -> table position (`single_rows` of a dense index, whose rows are not table positions once a
    chunk has no embedding; None: the ids are positions, as the sparse store's and a multi-vector store's are)."""
    codes: dict = {}
    by_pos = np.full(len(ids), -1, dtype=np.int64)
    for p, pk in enumerate(ids):
        src = source_of.get(pk)
        if src is not None:
            by_pos[p] = codes.setdefault(src, len(codes))
    return by_pos if pos_of_row is None else by_pos[np.asarray(pos_of_row, dtype=np.int64)]


class _SourceKeys(NamedTuple):   # one leg's key table on the device, and what it was built from (_UnitIndex.source_keys)
    source_of: Any
    table: ChunkTable
    rows: np.ndarray | None
    handle: Any          # the index whose device the block was taken on (under a _World: the sharded searcher's)
    ptr: int
    length: int


class DeviceLists(NamedTuple):
    """One leg's [B, width] lists where its search left them (`dense_lists_device` / `bm25_lists_device`): the handle and
    scratch they belong to, distances float64 and ids int64 as device pointers, how a distance becomes the leg's score
    (Mi355Index.fuse_lists `modes`), and the device map from the leg's ids to table positions (0 / 0: they are positions).
    Valid until the same leg's next page."""

    index: Mi355Index
    scratch: _DevScratch
    dist_ptr: int
    ids_ptr: int
    B: int
    width: int
    mode: str
    map_ptr: int
    map_len: int


class _UnitIndex:
    """GPU index of one table (chunk / image_chunk): row <-> primary-key mapping + the native handle."""

    def __init__(self, table: ChunkTable, device: int, compact_dead_fraction: float | None = None):
        self.table = table
        self.single: Mi355Index | None = None
        self.multi: Mi355Index | None = None
        # THE layout of the single-vector index: index row -> table position, strictly increasing.  Every NOT NULL position
        # has a slot; a NULL position has a removed slot or none
        self.single_rows: np.ndarray | None = None
        self.multi_rows: np.ndarray | None = None
        self.device = device
        self.single_sharded: Any | None = None      # ShardedSearcher over this rank's rows (a _World is active)
        self.multi_sharded: Any | None = None
        # True (after compact_single): the positions that were NULL at the compaction have no slot ON PURPOSE and refresh works
        # through the map.  False with such positions missing: built over NULL rows and never laid out (`_apply_single`)
        self.compacted = False
        # refresh compacts by itself once dead / size reaches this fraction, or the head of the index is dead (None: never)
        self.compact_dead_fraction = compact_dead_fraction
        self._pos_of_id = self._stored_row_of_pos = None   # (dict) caches of pos_of_id() / stored_row_of_pos(): see _forget_maps
        # the sparse store of `table.contents` under one tokenizer (BM25): document id = table position.  It is replicated, not
        # sharded, and brought up to the table's contents when they are no longer what it was built from (`ensure_sparse`)
        self.sparse: Mi355Index | None = None
        self._sparse_of: tuple[Any, list] | None = None    # (tokenizer key, the contents list it was built from)
        # ... unless the service was asked to shard it (`shard_sparse=True` under a _World): this rank's contiguous slice of the
        # positions behind a ShardedSearcher, global document id = table position all the same (`sparse_searcher`)
        self.sparse_sharded: Any | None = None
        self._sparse_sharded_of: tuple[Any, list] | None = None
        # device-side page buffers of the legs that leave their lists in HBM, and the device copy of `single_rows` they hand
        # the fusion as its map (`single_rows_device`; dropped with the other maps in _forget_maps)
        self.scratch = _DevScratch()
        self._single_rows_dev: tuple[np.ndarray, int, int] | None = None   # (the single_rows array it copies, pointer, length)
        # the `per_source` key tables, one per leg ("single" / "multi" / "sparse"), kept on the device while the mapping, the
        # table and the leg's layout are the objects they were built from (`source_keys`)
        self._source_keys: dict[str, _SourceKeys] = {}

    def _not_null_positions(self) -> np.ndarray:
        emb = self.table.embedding
        if emb is None:
            raise ValueError("table has no single-vector embeddings")
        return np.nonzero(~np.isnan(emb).all(axis=1))[0]  # WHERE embedding IS NOT NULL

    def single_positions(self) -> np.ndarray:
        """`single_rows`, without building an index: a unit nothing was laid out for has the NOT NULL rows in table order."""
        if self.single_rows is None:
            self.single_rows = self._not_null_positions()
        return self.single_rows

    def single_searcher(self, world: "_World | None") -> Any:
        """The local index -- or, under a world, this rank's contiguous share of the NOT NULL rows behind a ShardedSearcher
        (global row ids = positions in the table's not-null order, the same ids the unsharded index uses)."""
        if world is None:
            return self.ensure_single()
        if self.single_sharded is None:
            from .sharded import ShardedSearcher, shard_bounds  # noqa: PLC0415

            rows, emb = self.single_positions(), self.table.embedding
            lo, hi = shard_bounds(int(rows.shape[0]), world.size, world.rank)
            s = ShardedSearcher(emb.shape[1], "cosine", self.device, index_factory=Mi355Index, group=world.group)
            s.add_local(emb[rows[lo:hi]], lo)
            self.single_sharded = s
        return self.single_sharded

    def multi_searcher(self, world: "_World | None") -> Any:
        """Multi-vector table: under a world the docs are cut by cumulative TOKEN count (the MaxSim pass streams token rows:
        SURVEY 8(e))."""
        if world is None:
            return self.ensure_multi()
        if self.multi_sharded is None:
            from .sharded import ShardedSearcher, shard_bounds_by_tokens  # noqa: PLC0415

            tok, off = self.table.mv_tokens, self.table.mv_offsets
            if tok is None or off is None:
                raise ValueError("table has no multi-vector embeddings")
            lo, hi = shard_bounds_by_tokens(off, world.size, world.rank)
            s = ShardedSearcher(tok.shape[1], "cosine", self.device, index_factory=Mi355Index, group=world.group)
            s.add_local_multivec(tok[off[lo]:off[hi]], off[lo:hi + 1] - off[lo], lo)
            self.multi_sharded = s
            self.multi_rows = np.arange(off.shape[0] - 1)
        return self.multi_sharded

    def ensure_single(self) -> Mi355Index:
        if self.single is None:
            rows, emb = self.single_positions(), self.table.embedding
            self.single = Mi355Index(emb.shape[1], "cosine", self.device)
            self.single.add(emb if rows.shape[0] == emb.shape[0] else emb[rows])
        return self.single

    def ensure_multi(self) -> Mi355Index:
        if self.multi is None:
            tok, off = self.table.mv_tokens, self.table.mv_offsets
            if tok is None or off is None:
                raise ValueError("table has no multi-vector embeddings")
            self.multi = Mi355Index(tok.shape[1], "cosine", self.device)
            self.multi.add_multivec(tok, off)
            self.multi_rows = np.arange(off.shape[0] - 1)
        return self.multi

    def ensure_sparse(self, tokenizer: Any) -> Mi355Index:
        """The sparse store of the table's contents under `tokenizer` (a name or a callable, bm25.get_tokenizer): one document
        per table position, None = a document without tokens, so ids stay positions.  Built on first use.  A refresh that
        changed cells or appended rows is applied as the difference (`set_sparse` of the changed positions, `add_sparse` of the
        tail: only those are tokenised); a shorter table, another tokenizer, or a store object without `set_sparse` rebuilds it
        whole."""
        from .bm25 import get_tokenizer, tokenizer_key  # noqa: PLC0415

        key, contents = tokenizer_key(tokenizer), self.table.contents
        if self.sparse is not None and self._sparse_of is not None and self._sparse_of[0] == key:
            if self._sparse_of[1] is contents:
                return self.sparse
            if self._sparse_of[1] == contents:   # a newer export with the same contents: remember its list, compare once
                self._sparse_of = (key, contents)
                return self.sparse
        tok = get_tokenizer(tokenizer)

        def tokens(c):
            return [] if c is None else tok(c if isinstance(c, str) else bytes(c).decode("utf-8", "replace"))

        if (self.sparse is not None and self._sparse_of is not None and self._sparse_of[0] == key
                and len(self._sparse_of[1]) <= len(contents) and hasattr(self.sparse, "set_sparse")):
            # the table kept its positions and grew at the end at most: the difference alone -- one set of the cells that
            # changed, one add of the tail (under a process group every rank applies the same difference)
            old = self._sparse_of[1]
            changed = [i for i, c in enumerate(old) if c != contents[i]]
            if changed:
                self.sparse.set_sparse(changed, [tokens(contents[i]) for i in changed])
            if len(contents) > len(old):
                self.sparse.add_sparse([tokens(c) for c in contents[len(old):]])
            self._sparse_of = (key, contents)
            return self.sparse
        if self.sparse is not None:
            self.sparse.close()
            self.sparse = None
        docs = [tokens(c) for c in contents]
        ix = Mi355Index(8, "cosine", self.device)  # (the handle's dense side stays empty)
        ix.add_sparse(docs)
        self.sparse, self._sparse_of = ix, (key, contents)
        return ix

    def sparse_searcher(self, tokenizer: Any, world: "_World") -> Any:
        """`ensure_sparse` under a world, row-sharded: a ShardedSearcher over this rank's `shard_bounds` slice of the table
        positions (`row_offset` = the slice's start, the library communicator on `world.group`).  Its `search_bm25`,
        `search_bm25_subset` and `score_bm25_subset` take what the index's methods take and answer with the statistics of ALL
        ranks' documents.  Every rank sees the same table, so every rank takes the same branch: an equal-length table with
        changed cells is applied as `set_local_sparse` on the owners (the others have nothing to do, and the next search gathers
        the statistics anew); another length or another tokenizer rebuilds the store."""
        from .bm25 import get_tokenizer, tokenizer_key  # noqa: PLC0415
        from .sharded import ShardedSearcher, shard_bounds  # noqa: PLC0415

        key, contents = tokenizer_key(tokenizer), self.table.contents
        have, of = self.sparse_sharded, self._sparse_sharded_of
        if have is not None and of is not None and of[0] == key:
            if of[1] is contents:
                return have
            if of[1] == contents:
                self._sparse_sharded_of = (key, contents)
                return have
        tok = get_tokenizer(tokenizer)

        def tokens(c):
            return [] if c is None else tok(c if isinstance(c, str) else bytes(c).decode("utf-8", "replace"))

        lo, hi = shard_bounds(len(contents), world.size, world.rank)
        if have is not None and of is not None and of[0] == key and len(of[1]) == len(contents):
            changed = [i for i in range(lo, hi) if of[1][i] != contents[i]]
            if changed:
                have.set_local_sparse(changed, [tokens(contents[i]) for i in changed])
            self._sparse_sharded_of = (key, contents)
            return have
        if have is not None:
            have.close()
            self.sparse_sharded = None
        s = ShardedSearcher(8, "cosine", self.device, index_factory=Mi355Index, group=world.group)  # (the dense side stays empty)
        s.add_local_sparse([tokens(c) for c in contents[lo:hi]], lo)
        self.sparse_sharded, self._sparse_sharded_of = s, (key, contents)
        return s

    def _any_handle(self) -> Mi355Index | None:
        return next((ix for ix in (self.single, self.sparse, self.multi) if ix is not None), None)

    def source_keys(self, leg: str, source_of: Any, handle: Mi355Index) -> Any:
        """The device key table of a `per_source` search over one leg ("single": indexed by index rows through `single_rows`;
        "multi" / "sparse": by table position), built by `source_key_table` and uploaded ONCE per mapping: it is reused while
        `source_of` is the same object, the table and the layout are what it was built from and its block is still held.  A
        mapping changed in place is a stale one: pass a new object.  Returns a DeviceKeys that owns nothing."""
        from .index import DeviceKeys  # noqa: PLC0415

        rows = self.single_rows if leg == "single" else None
        name = "source_keys:" + leg
        have = self._source_keys.get(leg)
        if (have is None or have.source_of is not source_of or have.table is not self.table or have.rows is not rows
                or not self.scratch.holds(name, have.ptr)):
            host = np.ascontiguousarray(source_key_table(self.table.ids, source_of, rows))
            ptr = self.scratch.take(handle, name, max(host.nbytes, 8))
            if host.nbytes:
                handle.dev_upload(ptr, host)
            have = self._source_keys[leg] = _SourceKeys(source_of, self.table, rows, handle, ptr, host.shape[0])
        return DeviceKeys.borrowed(have.ptr if have.length else 0, have.length)

    def single_rows_device(self) -> tuple[int, int]:
        """(device pointer, length) of `single_rows` as int64: index row -> table position, the fusion's map for the dense
        leg.  Uploaded once per layout."""
        ix, rows = self.ensure_single(), self.single_rows
        if self._single_rows_dev is None or self._single_rows_dev[0] is not rows:
            host = np.ascontiguousarray(rows, dtype=np.int64)
            ptr = self.scratch.take(ix, "single_rows", max(host.nbytes, 8))
            if host.nbytes:
                ix.dev_upload(ptr, host)
            self._single_rows_dev = (rows, ptr, host.shape[0])
        return self._single_rows_dev[1:]

    def close(self) -> None:
        for leg, have in self._source_keys.items():   # (through the handle that took them: under a _World there is no local one)
            if self.scratch.holds("source_keys:" + leg, have.ptr):
                self.scratch.drop(have.handle, "source_keys:" + leg)
        self._source_keys.clear()
        self.scratch.release(self._any_handle())
        self._single_rows_dev = None
        for ix in (self.single, self.multi, self.single_sharded, self.multi_sharded, self.sparse, self.sparse_sharded):
            if ix is not None:
                ix.close()
        self.single = self.multi = self.single_sharded = self.multi_sharded = self.sparse = self.sparse_sharded = None
        self._sparse_of = self._sparse_sharded_of = None
        self._start_over(self.table)

    # ---- primary key -> table position -> index row (the GQR pools and the candidate scorer name chunks by key) ----
    def pos_of_id(self) -> dict:
        if self._pos_of_id is None:
            self._pos_of_id = {pk: i for i, pk in enumerate(self.table.ids)}
        return self._pos_of_id

    def stored_row_of_pos(self) -> dict:
        """table position -> index row, for the positions whose embedding is STORED.  Not `_slot_of_pos`: a refreshed unit
        keeps a slot for a NULL embedding -- a removed row that still holds a vector -- and that is not a stored one."""
        if self._stored_row_of_pos is None:
            stored = self._not_null_positions()
            self._stored_row_of_pos = dict(zip(stored.tolist(), self._slot_of_pos()[stored].tolist()))
        return self._stored_row_of_pos

    def _slot_of_pos(self) -> np.ndarray:
        """table position -> index row for EVERY position that has a slot, live or removed (-1: no slot): what a refresh
        addresses -- updating a removed slot is how a NULL is revived."""
        rows, slot = self.single_positions(), np.full(len(self.table.ids), -1, dtype=np.int64)
        slot[rows] = np.arange(rows.shape[0])
        return slot

    def _forget_maps(self) -> None:   # (the caches of pos_of_id / stored_row_of_pos: stale once the table or the layout changes)
        self._pos_of_id = self._stored_row_of_pos = None
        self._single_rows_dev = None      # (the device copy of single_rows; its block stays in `scratch` for the next one)

    @property
    def slot_per_position(self) -> bool:
        """There is a slot for every table position (NULL rows are removed slots, `single_rows` is the identity)."""
        return self.single_rows is not None and self.single_rows.shape[0] == len(self.table.ids)

    # ---- following the table ----
    def _start_over(self, table: ChunkTable) -> None:
        """Take `table` and forget everything derived from the old one: the row maps, the key maps, the layout flag."""
        self.table = table
        self.single_rows = self.multi_rows = None
        self.compacted = False
        self._forget_maps()

    def _relayout(self, emb: np.ndarray, null: np.ndarray, why: str) -> str:
        """`single` anew with one slot per table position: NULL rows are added as placeholders and removed at once."""
        logger.info("refresh: %s; laying it out with one slot per table position", why)
        self.scratch.release(self.single)
        self._single_rows_dev = None
        self.single.close()
        self.single = Mi355Index(emb.shape[1], "cosine", self.device)
        self._append_slots(emb, null, 0)
        self.single_rows = np.arange(emb.shape[0])
        self.compacted = False
        return "relayout"

    def _append_slots(self, emb: np.ndarray, null: np.ndarray, first: int) -> None:
        if emb.shape[0] == 0:
            return
        self.single.add(np.where(null[:, None], np.float32(0), emb) if null.any() else emb)
        if null.any():
            self.single.remove_rows(first + np.nonzero(null)[0])

    def _rebuild(self, table: ChunkTable, why: str) -> str:
        logger.info("refresh: full rebuild of the index (%s)", why)
        self.close()
        self._start_over(table)
        return "rebuild"

    # ---- compaction (Mi355Index.compact: the removed slots are squeezed out in place, the live rows keep their order) ----
    def compact_single(self) -> bool:
        """Drop the removed slots of the single-vector index.  Acts when that index is built, the unit is not row-sharded and
        the index has dead rows; True when it acted.  Afterwards the unit holds slots for the NOT NULL positions only, still
        in table order (`single_rows` strictly increasing), and `refresh` keeps following the table in place through that
        map.  Exact distance ties break as in a unit built fresh from the table."""
        if self.single is None or self.single_sharded is not None or len(self.single) == self.single.live_rows:
            return False
        new_of_old = np.asarray(self.single.compact())
        self.single_rows = np.asarray(self.single_rows)[new_of_old >= 0]
        self._forget_maps()
        self.compacted = True
        return True

    _HEAD_SLOTS, _HEAD_LIVE = 65536, 1024   # the dead-head condition: fewer than _HEAD_LIVE of the first _HEAD_SLOTS slots live

    def _wants_compaction(self, null: np.ndarray) -> bool:
        """The policy of `compact_dead_fraction`, from the NULL pattern of the table just applied (a slot is live exactly
        when its position is NOT NULL).  Dead head: a search pass takes its first threshold from the first slots of the
        index (DESIGN "Known cliff").  A table with fewer than 1024 live rows in its head meets that condition with any dead
        row: at that size a compaction costs less than the fallbacks it avoids."""
        if self.compact_dead_fraction is None:
            return False
        size = len(self.single)
        dead = size - self.single.live_rows
        if dead == 0:
            return False
        if dead >= self.compact_dead_fraction * size:
            return True
        head = np.asarray(self.single_rows)[:min(size, self._HEAD_SLOTS)]
        return int((~null[head]).sum()) < self._HEAD_LIVE

    def refresh(self, table: ChunkTable) -> str:
        """Follow a newer export of the same table.  With the same primary keys in the same order (new keys only at the end)
        the live indexes take the difference alone.  The single-vector index -- what the reference's `UPDATE ... SET embedding`
        (orm/service/base_ingestion.py:199-247) and `WHERE embedding IS NOT NULL` (orm/repository/base.py:409-415) make of it:

            embedding changed -> update_rows        embedding became NULL -> remove_rows
            NULL became a vector -> update_rows (the slot is revived)     new keys at the end -> add

        The multi-vector index (`set_multi_vector_embedding(s_batch)`, orm/repository/base.py:428-485, and `embeddings IS NOT
        NULL`, :487-535), when it is built and both exports carry the column with the same width:

            token count or token bits changed, vectors lost, vectors regained -> ONE set_multivec (no vectors = removed)
            new keys at the end -> ONE add_multivec

        A unit with both indexes built takes both differences; one with only the multi-vector index built takes that one (the
        single-vector index is built from `table` when first asked for, and "unchanged" means neither column changed).

        Row mapping: `single_rows` is the layout and the difference is applied through it (`_apply_single`): a row that
        becomes NULL keeps its slot, removed; new keys get slots at the end.  An index built over NULL rows is laid out anew
        ONCE -- one slot per table position, NULL rows being removed slots -- at the first refresh that changes the column (the
        only rebuild on this path).  Slots stay in table order throughout, so exact distance ties break as in a unit built
        fresh from `table`.  The multi-vector index always has one document per table position (`multi_rows` = the identity).

        A changed key order, a changed width, a multi-vector column that appears or disappears (or one no index was built
        for) and row-sharded units (one process per GPU) fall back to the full rebuild (close; the next search builds from
        `table`).  Returns "deferred" (nothing built yet), "unchanged", "incremental", "relayout", "rebuild" or -- only with
        `compact_dead_fraction` set -- "compacted": applied in place, the removed slots then squeezed out (`compact_single`)."""
        old = self.table
        if self.single is None and self.multi is None and self.single_sharded is None and self.multi_sharded is None:
            self._start_over(table)
            return "deferred"
        if table.mv_offsets is not None or old.mv_offsets is not None or self.multi is not None or self.multi_sharded is not None:
            if self.multi_sharded is not None or self.single_sharded is not None:
                return self._rebuild(table, "multi-vector unit: row-sharded stores are not followed in place")
            if self.multi is None or table.mv_offsets is None or old.mv_offsets is None:
                return self._rebuild(table, "multi-vector unit: the column appeared or disappeared, or no index was built for it")
        if self.single_sharded is not None:
            return self._rebuild(table, "row-sharded unit: global row ids are positions in the not-null order")
        n_old = len(old.ids)
        if len(table.ids) < n_old or list(table.ids[:n_old]) != list(old.ids):
            return self._rebuild(table, "the primary keys or their order changed")
        # ---- what each built index has to do (nothing is touched before both differences are known to be applicable)
        single_plan = multi_plan = None
        if self.single is not None:
            emb, was = table.embedding, old.embedding
            if emb is None or was is None or emb.shape[1] != was.shape[1]:
                return self._rebuild(table, "the embedding column changed shape")
            single_plan = self._single_difference(np.ascontiguousarray(emb, dtype=np.float32),
                                                  np.ascontiguousarray(was, dtype=np.float32), n_old)
        if self.multi is not None:
            if table.mv_tokens is None or old.mv_tokens is None or table.mv_tokens.shape[1] != old.mv_tokens.shape[1]:
                return self._rebuild(table, "the multi-vector column changed width")
            multi_plan = self._multi_difference(table, old, n_old)
        self._forget_maps()
        appended = len(table.ids) > n_old
        single_changes = single_plan is not None and (single_plan.update.any() or single_plan.remove.any() or appended)
        multi_changes = multi_plan is not None and (multi_plan.changed.size > 0 or appended)
        if self.single is None:
            # no single-vector index to follow: it is built from `table` when first asked for, and positions cached from the
            # old table's NULL pattern (`single_positions`) do not outlive that table
            self.single_rows = None
            if not multi_changes and not self._same_bits(table.embedding, old.embedding):
                self.table = table
                return "incremental"                                             # ("unchanged" means neither column changed)
        if not (single_changes or multi_changes):
            self.table = table
            return "unchanged"
        outcome = "incremental"
        if single_changes:
            outcome = self._apply_single(single_plan, n_old)
            if outcome == "incremental" and self._wants_compaction(single_plan.null) and self.compact_single():
                outcome = "compacted"
        if multi_changes:
            self._apply_multi(table, multi_plan, n_old)
        self.table = table
        if self.multi is not None:
            self.multi_rows = np.arange(len(table.ids))
        return outcome

    @staticmethod
    def _same_bits(a: np.ndarray | None, b: np.ndarray | None) -> bool:
        if a is None or b is None:
            return a is None and b is None
        a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
        return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())      # (bits: NaN-safe)

    @staticmethod
    def _single_difference(emb: np.ndarray, was: np.ndarray, n_old: int) -> _SinglePlan:
        null, was_null = np.isnan(emb).all(axis=1), np.isnan(was).all(axis=1)
        head, head_null = emb[:n_old], null[:n_old]
        differ = (head.view(np.uint32) != was.view(np.uint32)).any(axis=1)      # (bits: NaN-safe)
        return _SinglePlan(emb=emb, null=null, was_null=was_null, update=~head_null & (was_null | differ),
                           remove=head_null & ~was_null)

    def _apply_single(self, plan: _SinglePlan, n_old: int) -> str:
        """Apply the difference through `single_rows` and its inverse (`_slot_of_pos`; `self.table` is still the old table
        here).  An index this call does not touch keeps its layout."""
        emb, null = plan.emb, plan.null
        slot = self._slot_of_pos()
        update, remove = np.nonzero(plan.update)[0], np.nonzero(plan.remove)[0]
        if not self.compacted and self.single_rows.shape[0] < n_old:
            # KEPT ON PURPOSE (the routine below could serve this unit in place wherever no NULL row regains a vector): a unit
            # built over NULL rows and never compacted lays itself out at the first change of the column, whatever the change
            return self._relayout(emb, null, "the index was built over NULL rows")
        if (slot[update] < 0).any():   # (its slot would have to lie between two others to keep table order)
            return self._relayout(emb, null, "a NULL row without a slot in the compacted index regained a vector")
        if remove.size:
            self.single.remove_rows(slot[remove])
        if update.size:
            self.single.update_rows(slot[update], emb[update])
        self._append_slots(emb[n_old:], null[n_old:], len(self.single))
        self.single_rows = np.concatenate([self.single_rows, np.arange(n_old, emb.shape[0])])
        return "incremental"

    @staticmethod
    def _multi_difference(table: ChunkTable, old: ChunkTable, n_old: int) -> _MultiPlan:
        """Positions < n_old whose documents differ between the two exports: another token count (losing or regaining every
        vector included) or, at the same count, other token bits."""
        off = np.ascontiguousarray(table.mv_offsets, dtype=np.int64)
        was_off = np.ascontiguousarray(old.mv_offsets, dtype=np.int64)
        tok = np.ascontiguousarray(table.mv_tokens, dtype=np.float32)
        was_tok = np.ascontiguousarray(old.mv_tokens, dtype=np.float32)
        lens, was_lens = np.diff(off[:n_old + 1]), np.diff(was_off)
        changed = lens != was_lens
        same = np.nonzero(~changed & (lens > 0))[0]
        if same.size:
            n = lens[same]
            first = np.cumsum(n) - n                                             # of each such document in the gathered rows
            within = np.arange(int(n.sum())) - np.repeat(first, n)
            rows, was_rows = np.repeat(off[same], n) + within, np.repeat(was_off[same], n) + within
            differ = (tok[rows].view(np.uint32) != was_tok[was_rows].view(np.uint32)).any(axis=1)   # (bits: NaN-safe)
            changed[same[np.logical_or.reduceat(differ, first)]] = True
        return _MultiPlan(off=off, tok=tok, changed=np.nonzero(changed)[0])

    def _apply_multi(self, table: ChunkTable, plan: _MultiPlan, n_old: int) -> None:
        off, tok, ids = plan.off, plan.tok, plan.changed
        if ids.size:
            lens = off[ids + 1] - off[ids]
            parts = [tok[off[i]:off[i + 1]] for i in ids]
            self.multi.set_multivec(ids, np.concatenate(parts, axis=0) if parts else tok[:0],
                                    np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
        if len(table.ids) > n_old:
            self.multi.add_multivec(tok[off[n_old]:off[-1]], off[n_old:] - off[n_old])


def _is_store(obj: Any) -> bool:
    return all(hasattr(obj, a) for a in ("get_or_create_pipeline", "get_all_queries", "completed_query_ids", "chunks"))


class Mi355RetrievalService:
    """`session_factory` is what the caller of the pipeline passes:

    * a callable returning a store (InMemoryStore, or any object with that interface) -- standalone use, bench, tests;
    * a SQLAlchemy `sessionmaker`, which is what the reference's Executor and its wrapper pipelines pass
      (executor.py:326-333, hybrid.py `_load_pipeline`).  The service then builds the reference's own
      `RetrievalPipelineService(session_factory, schema)` and reads / writes the database through it (store.UowStore);
      that needs the `autorag_research` package importable, which it is wherever the Executor runs.
    """

    def __init__(self, session_factory: Callable[[], Any], schema: Any | None = None, device: int = 0,
                 compact_dead_fraction: float | None = None, shard_sparse: bool = False):
        self.session_factory = session_factory
        # True: under a _World the chunk table's sparse store (BM25) is row-sharded over the ranks like the dense index, and
        # the lexical searches run the library's sharded forms (global N / avgdl / df, gathered per call).  False, or without a
        # _World: every rank holds the whole store, as before
        self._shard_sparse = bool(shard_sparse)
        # None: units never compact by themselves (compact_unit still does); else `_UnitIndex.refresh` compacts the single-vector
        # index once that share of its slots is dead, or its head is
        self._compact_dead_fraction = compact_dead_fraction
        self._schema = schema
        # one process per GPU under torch.distributed: this rank's GPU, row-sharded units, rank 0 reads ids / writes results
        self._world = _World.detect()
        if self._world is not None:
            device = int(os.environ.get("LOCAL_RANK", device))
            self._world.bind_device(device)
        self._device = device
        self._units: dict[str, _UnitIndex] = {}
        self._uow_store: UowStore | None = None
        probe = session_factory()
        if not _is_store(probe):
            close = getattr(probe, "close", None)
            if callable(close):
                close()
            try:
                from autorag_research.orm.service.retrieval_pipeline import RetrievalPipelineService  # noqa: PLC0415
            except ImportError as e:  # pragma: no cover - only outside a reference installation
                raise TypeError(
                    f"session_factory() returned a {type(probe).__name__}, not a store; a SQLAlchemy sessionmaker is served "
                    "through the reference's RetrievalPipelineService, which needs `autorag_research` importable") from e
            self._uow_store = UowStore(RetrievalPipelineService(session_factory, schema), require_total_order=self._world is not None)

    # ---- plumbing ----
    def _store(self) -> Any:
        return self._uow_store if self._uow_store is not None else self.session_factory()

    def from_root(self, make: Callable[[], Any]) -> Any:
        """`make()` -- under a _World on rank 0 only, its value (or its exception) on every rank (`_World.from_root`).  This,
        `on_root`, `agree` and `_same_table_everywhere` are the only places that ask "one process per GPU, or not"."""
        return make() if self._world is None else self._world.from_root(make)

    async def on_root(self, make: Callable[[], Awaitable[Any]]) -> Any:
        """`await make()`, shared the same way: an embedding-model call is a rank-local step that may fail or differ."""
        if self._world is None:
            return await make()
        outcome = None
        if self._world.rank == 0:
            try:
                outcome = (True, await make())
            except Exception as e:  # noqa: BLE001 - re-raised by share_outcome, on every rank
                outcome = (False, _World._portable(e))
        return self._world.share_outcome(outcome)

    def agree(self, ok: bool) -> bool:
        """True iff `ok` on every rank (`_World.agree`); `ok` itself in a single process."""
        return ok if self._world is None else self._world.agree(ok)

    def _same_table_everywhere(self, unit: str, table: ChunkTable) -> None:
        """Every rank exported the table by itself: global row ids are positions in the export order, so the ranks must have
        seen the SAME keys in the SAME order with the same NULL pattern before any of them shards or follows it."""
        if self._world is not None:
            self._world.same_everywhere(f"table {unit!r}", _table_digest(table))

    def delete_pipeline_results(self, pipeline_id) -> int:
        """Reference RetrievalPipelineService.delete_pipeline_results (:359-372): the Executor's health-check cleanup."""
        return self.from_root(lambda: self._store().delete_pipeline_results(pipeline_id))

    def _unit(self, unit: str) -> _UnitIndex:
        if unit not in self._units:
            store = self._store()
            table = store.image_chunks if unit == "image_chunk" else store.chunks
            self._same_table_everywhere(unit, table)
            self._units[unit] = _UnitIndex(table, self._device, self._compact_dead_fraction)
        return self._units[unit]

    def refresh_unit(self, unit: str, table: ChunkTable) -> str:
        """Hand a unit a newer export of its table: the live index takes the difference alone where it can
        (`_UnitIndex.refresh`).  A unit nothing was built for yet reads the store's table at its first search, as before."""
        if unit not in self._units:
            return "deferred"
        self._same_table_everywhere(unit, table)
        return self._units[unit].refresh(table)

    def compact_unit(self, unit: str) -> bool:
        """Squeeze the removed slots out of a unit's single-vector index now (`_UnitIndex.compact_single`); False when there
        was nothing to do: no such unit or index yet, a row-sharded unit, or no removed slot."""
        return unit in self._units and self._units[unit].compact_single()

    def get_queries(self, query_ids: list) -> list:
        """The stored query rows (None = no such query).  One process per GPU: rank 0 reads them and every rank gets the same
        rows -- a transient database error then happens once, on rank 0, and reaches every rank as the same exception instead
        of sending one rank down the retry path while the others wait in the block's collective."""
        return self.from_root(lambda: [self._store().get_query(q) for q in query_ids])

    def close(self) -> None:
        for u in self._units.values():
            u.close()
        self._units.clear()
        if getattr(self, "_scratch", None) is not None:
            self._scratch.close()
            self._scratch = None

    def get_or_create_pipeline(self, name: str, config: dict[str, Any]) -> tuple[int, bool]:
        # (one process per GPU: one row in the pipeline table, created by rank 0)
        return self.from_root(lambda: tuple(self._store().get_or_create_pipeline(name, config)))

    def find_query_by_text(self, query_text: str):
        return self.from_root(lambda: self._store().find_query_by_text(query_text))

    def _make_retrieval_result(self, table: ChunkTable, pos: int, score: float, with_content: bool) -> dict[str, Any]:
        return {"doc_id": table.ids[pos], "score": score, "content": table.contents[pos] if with_content else None}

    # ---- the hot path ----
    def vector_search(self, query_ids: list[int | str], top_k: int = 10,
                      search_mode: Literal["single", "multi"] = "single", unit: str = "chunk",
                      within: list | None = None, mmr_fetch_k: int | None = None,
                      mmr_lambda: float = 0.5, per_source: int | None = None, source_of: Any = None,
                      source_fetch_k: int | None = None) -> list[list[dict]]:
        """Top-k for every query id, scored as one block.  Raises ValueError exactly like the reference.
        `within` (not in the reference's signature; None = today's behaviour): primary keys the search is restricted to --
        the statement with `AND id = ANY(:within)`.  Keys unknown to the table or without a stored embedding are left out.
        `mmr_fetch_k` (None = today's behaviour; single mode only): diversify -- the top_k results are picked from the
        mmr_fetch_k nearest by Maximal Marginal Relevance with weight `mmr_lambda` on the query similarity
        (Mi355Index.search_mmr), and come in selection order.
        `per_source` (None = today's behaviour): at most that many results per source -- `source_of` maps a primary key to
        its source (a document, a page, a duplicate cluster; a missing key has none and is never capped).  Single mode
        without `within`: Mi355Index.search_collapsed, which deepens only the queries whose cap bites (first round at
        `source_fetch_k`, default `Mi355Index.collapse_fetch_k`) and so returns top_k results wherever the first 1024 of the
        ranking hold them; with `within` and in multi mode: ONE search at `source_fetch_k` (default LIST_SOURCE_FETCH_MULT *
        top_k, at most 1024), then the cap over its lists -- nothing deepens there, so a query whose cap strikes more than
        that depth can refill gets fewer than top_k results.  Not together with `mmr_fetch_k`."""
        self._check_mmr(search_mode, mmr_fetch_k)
        self._check_per_source(top_k, per_source, source_of, source_fetch_k, mmr_fetch_k)
        queries = []
        for qid, q in zip(query_ids, self.get_queries(list(query_ids)), strict=True):
            if q is None:
                raise ValueError(f"Query {qid} not found")  # noqa: TRY003
            if search_mode == "multi":
                if q.embeddings is None:
                    raise ValueError(f"Query {qid} has no multi-vector embeddings")  # noqa: TRY003
            elif q.embedding is None:
                msg = f"Query {qid} has no embedding" if unit == "chunk" else f"Query {qid} has no single-vector embedding"
                raise ValueError(msg)
            queries.append(q)
        if not queries:
            return []
        if search_mode == "multi":
            return self.maxsim_search_by_embeddings([q.embeddings for q in queries], top_k, unit, within=within,
                                                    per_source=per_source, source_of=source_of, source_fetch_k=source_fetch_k)
        Q = np.stack([q.embedding for q in queries]).astype(np.float32, copy=False)
        return self._single_block(Q, top_k, unit, within, mmr_fetch_k, mmr_lambda, per_source, source_of, source_fetch_k)

    # ---- BM25: the lexical leg, over the unit's sparse store (reference retrieval_pipeline.py:398-465) ----
    def _sparse_store(self, u: _UnitIndex, tokenizer: Any) -> Any:
        """The unit's sparse store: the whole table on this rank, or -- `shard_sparse=True` under a _World -- the row-sharded
        searcher, whose BM25 methods take the same arguments and return the same lists on every rank."""
        if self._shard_sparse and self._world is not None:
            return u.sparse_searcher(tokenizer, self._world)
        return u.ensure_sparse(tokenizer)

    def _bm25_block(self, texts: list[str], top_k: int, tokenizer: Any, k1: float, b: float,
                    within: list | None = None, per_source: int | None = None, source_of: Any = None,
                    source_fetch_k: int | None = None) -> list[list[dict]]:
        """A page of query texts as one block.  Under a process group every rank holds the whole sparse store and computes the
        same lists -- or, with `shard_sparse=True`, its slice of it, and the library's sharded search returns the same lists.
        score = -distance: positive, higher is better, as the reference negates the operator's (chunk.py:236).
        `within`: among the listed keys only -- a filter under the whole store's statistics, as the reference's statement
        with `AND id = ANY(:ids)` behaves; unknown keys are left out.  `per_source`: ONE search at `source_fetch_k` (default
        LIST_SOURCE_FETCH_MULT * top_k), then at most that many per source: nothing deepens, a list can come back shorter
        than top_k (`vector_search`)."""
        from .bm25 import get_tokenizer  # noqa: PLC0415

        self._check_per_source(top_k, per_source, source_of, source_fetch_k, None)
        u = self._unit("chunk")
        ix = self._sparse_store(u, tokenizer)
        tok = get_tokenizer(tokenizer)
        queries = [tok(t) for t in texts]
        depth = top_k if per_source is None else self._source_depth(top_k, source_fetch_k)
        if within is None:
            dist, rows = ix.search_bm25(queries, depth, k1=k1, b=b)
        else:
            dist, rows = self._bm25_within(u, ix, queries, depth, k1, b, within)
        if per_source is not None:
            dist, rows = self._cap_lists(u, "sparse", ix, dist, rows, per_source, source_of, top_k)
        return self._results_from_block(u.table, np.arange(len(u.table.ids)), rows, -dist, True)

    @staticmethod
    def _bm25_within(u: _UnitIndex, ix: Any, queries: list, top_k: int, k1: float, b: float, within: list):
        """`search_bm25` among the listed keys (sparse id = table position).  One `search_bm25_subset` call where the store has
        it; a store object without it searches everything (k = size_sparse()) and the host strikes out the rest: the same
        lists."""
        pos = u.pos_of_id()
        docs = np.array(sorted({pos[pk] for pk in within if pk in pos}), dtype=np.int64)
        dist = np.full((len(queries), top_k), np.nan, dtype=np.float64)
        rows = np.full((len(queries), top_k), -1, dtype=np.int64)
        if docs.size and hasattr(ix, "search_bm25_subset"):
            return ix.search_bm25_subset(queries, top_k, docs, k1=k1, b=b)
        if docs.size and ix.size_sparse() > 0:
            d, r = ix.search_bm25(queries, ix.size_sparse(), k1=k1, b=b)
            for j in range(len(queries)):
                keep = np.flatnonzero(np.isin(r[j], docs) & (r[j] >= 0))[:top_k]
                dist[j, :keep.size], rows[j, :keep.size] = d[j, keep], r[j, keep]
        return dist, rows

    def bm25_score_candidates(self, query_text: str, doc_ids: list, tokenizer: Any = "simple", k1: float = 1.2,
                              b: float = 0.75) -> dict:
        """BM25 score of explicit candidates: {doc_id: positive score}, the score `bm25_search_by_text` gives the same chunk.
        Ids unknown to the table and candidates that hold no query term are left out (as `maxsim_score_candidates` does)."""
        from .bm25 import get_tokenizer  # noqa: PLC0415

        u = self._unit("chunk")
        ix = self._sparse_store(u, tokenizer)
        pos = u.pos_of_id()
        known = [(pk, pos[pk]) for pk in doc_ids if pk in pos]
        if not known:
            return {}
        rows = np.array([[p for _, p in known]], dtype=np.int64)
        dist = ix.score_bm25_subset([get_tokenizer(tokenizer)(query_text)], rows, k1=k1, b=b)[0]
        return {pk: -float(dv) for (pk, _), dv in zip(known, dist) if dv == dv}

    def bm25_search(self, query_ids: list[int | str], top_k: int = 10, tokenizer: Any = "simple",
                    index_name: str = "idx_chunk_bm25", k1: float = 1.2, b: float = 0.75,
                    per_source: int | None = None, source_of: Any = None, source_fetch_k: int | None = None,
                    within: list | None = None) -> list[list[dict]]:
        """BM25 top-k for every query id, scored as one block (reference bm25_search, :425-465; `index_name` is recorded by the
        pipeline and unused here).  Raises ValueError exactly like the reference.  `within`: among the listed chunk ids only.
        `per_source` / `source_of` / `source_fetch_k`: at most that many results per source, as in `vector_search`'s list-capped
        legs.  They stand BEFORE `within` in the signature: pass `within` by keyword."""
        texts = []
        for qid, q in zip(query_ids, self.get_queries(list(query_ids)), strict=True):
            if q is None:
                raise ValueError(f"Query {qid} not found")  # noqa: TRY003
            texts.append(q.contents or "")
        if not texts:
            return []
        return self._bm25_block(texts, top_k, tokenizer, k1, b, within, per_source, source_of, source_fetch_k)

    def bm25_search_by_text(self, query_text: str, top_k: int = 10, tokenizer: Any = "simple",
                            index_name: str = "idx_chunk_bm25", k1: float = 1.2, b: float = 0.75,
                            per_source: int | None = None, source_of: Any = None, source_fetch_k: int | None = None,
                            within: list | None = None) -> list[dict]:
        """BM25 top-k of a raw query text, no query row needed (reference bm25_search_by_text, :398-423).  `within`: among the
        listed chunk ids only.  `per_source` / `source_of` / `source_fetch_k`: as in `bm25_search` (before `within`: pass
        `within` by keyword)."""
        return self._bm25_block([query_text], top_k, tokenizer, k1, b, within, per_source, source_of, source_fetch_k)[0]

    # ---- hybrid fusion on the device: both legs' lists stay in HBM (include/mi355dr.h "hybrid fusion") ----
    def dense_lists_device(self, Q: np.ndarray, top_k: int) -> DeviceLists | None:
        """`_single_block` of the chunk table that leaves distances and rows on the device (one `search_device`).  None where
        the lists could differ from the host path's or cannot be had: a process group, top_k above the search's 1024, a
        query or stored row whose distance is NaN (the host path keeps such results, the fusion strikes them out)."""
        if self._world is not None or not 0 < top_k <= 1024:
            return None
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        norms = np.einsum("ij,ij->i", Q.astype(np.float64), Q.astype(np.float64))
        if not (np.isfinite(norms).all() and (norms > 0).all()):
            return None
        u = self._unit("chunk")
        ix = u.ensure_single()
        if ix.stat("irregular_rows") != 0:
            return None
        B = Q.shape[0]
        q_ptr = u.scratch.take(ix, "dense_q", Q.nbytes)
        dist_ptr = u.scratch.take(ix, "dense_dist", B * top_k * 8)
        rows_ptr = u.scratch.take(ix, "dense_rows", B * top_k * 8)
        ix.dev_upload(q_ptr, Q)
        ix.search_device(q_ptr, B, top_k, dist_ptr, rows_ptr)
        map_ptr, map_len = u.single_rows_device()
        return DeviceLists(ix, u.scratch, dist_ptr, rows_ptr, B, top_k, "one_minus", map_ptr, map_len)

    def bm25_lists_device(self, texts: list[str], top_k: int, tokenizer: Any, k1: float, b: float) -> DeviceLists | None:
        """`_bm25_block` that leaves distances and ids (= table positions) on the device (one `search_bm25_device`)."""
        from .bm25 import get_tokenizer  # noqa: PLC0415

        if self._world is not None or not 0 < top_k <= 1024:
            return None
        u = self._unit("chunk")
        ix = u.ensure_sparse(tokenizer)
        if not hasattr(ix, "search_bm25_device"):
            return None
        tok = get_tokenizer(tokenizer)
        B = len(texts)
        dist_ptr = u.scratch.take(ix, "bm25_dist", B * top_k * 8)
        ids_ptr = u.scratch.take(ix, "bm25_ids", B * top_k * 8)
        ix.search_bm25_device([tok(t) for t in texts], top_k, dist_ptr, ids_ptr, k1=k1, b=b)
        return DeviceLists(ix, u.scratch, dist_ptr, ids_ptr, B, top_k, "negate", 0, 0)

    @staticmethod
    def fuse_device_lists(lists_1: DeviceLists, lists_2: DeviceLists, table: ChunkTable, top_k: int, **spec) -> list[list[dict]]:
        """Two legs' device lists -> the dicts `hybrid.rrf_fuse` / `hybrid.cc_fuse` return ({"doc_id", "score"}, doc_id from
        the table position): one fusion launch on the first leg's handle (the lists may be two services' handles on one GPU),
        one [B, top_k] download.  `spec`: Mi355Index.fuse_lists' method / rrf_k / fetch_k / weight / mins."""
        ix, B = lists_1.index, lists_1.B
        if lists_2.B != B:
            raise ValueError("the two legs answered different numbers of queries")
        out_v = np.empty((B, top_k), dtype=np.float64)
        out_i = np.empty((B, top_k), dtype=np.int64)
        v_ptr = lists_1.scratch.take(ix, "fused_scores", max(out_v.nbytes, 8))
        i_ptr = lists_1.scratch.take(ix, "fused_ids", max(out_i.nbytes, 8))
        ix.fuse_lists_device(lists_1.dist_ptr, lists_1.ids_ptr, lists_1.width, lists_2.dist_ptr, lists_2.ids_ptr, lists_2.width,
                             B, top_k, v_ptr, i_ptr, None, modes=(lists_1.mode, lists_2.mode),
                             map1_ptr=lists_1.map_ptr or None, map1_len=lists_1.map_len,
                             map2_ptr=lists_2.map_ptr or None, map2_len=lists_2.map_len, **spec)
        if B == 0:
            return []
        ix.dev_download(v_ptr, out_v)
        ix.dev_download(i_ptr, out_i)
        neg = out_i < 0
        n_valid = np.where(neg.any(axis=1), neg.argmax(axis=1), top_k).tolist()
        pos, sc, ids = out_i.tolist(), out_v.tolist(), table.ids
        return [[{"doc_id": ids[p], "score": s} for p, s in zip(pr[:n], sr[:n])] for pr, sr, n in zip(pos, sc, n_valid)]

    def _check_mmr(self, search_mode: str, mmr_fetch_k: int | None) -> None:
        """MMR is a single-vector, single-GPU selection: it scores stored rows against each other, and under row shards the
        candidates' vectors lie on different GPUs.  Raised on every rank alike, before any collective."""
        if mmr_fetch_k is None:
            return
        if search_mode == "multi":
            raise ValueError("mmr_fetch_k applies to search_mode='single' only")  # noqa: TRY003
        if self._world is not None:
            raise NotImplementedError("MMR under a process group: the candidates' vectors lie on different GPUs")

    @staticmethod
    def _check_per_source(top_k: int, per_source: int | None, source_of: Any, source_fetch_k: int | None,
                          mmr_fetch_k: int | None) -> None:
        """The `per_source` arguments of every search method, checked before anything is searched (on every rank alike)."""
        if per_source is None:
            return
        if isinstance(per_source, bool) or not isinstance(per_source, (int, np.integer)) or per_source < 1:
            raise ValueError("per_source must be an integer >= 1")  # noqa: TRY003
        if source_of is None or not hasattr(source_of, "get"):
            raise ValueError("per_source needs source_of, a mapping from primary key to source")  # noqa: TRY003
        if mmr_fetch_k is not None:
            raise ValueError("per_source and mmr_fetch_k are two selections over one list: pass one of them")  # noqa: TRY003
        if source_fetch_k is not None and not top_k <= source_fetch_k <= 1024:
            raise ValueError("source_fetch_k must lie in [top_k, 1024]")  # noqa: TRY003

    @staticmethod
    def _source_depth(top_k: int, source_fetch_k: int | None) -> int:
        """The depth the LIST-capped legs (`within`, MaxSim, BM25) search at: `source_fetch_k`, or LIST_SOURCE_FETCH_MULT *
        top_k within [top_k, 1024].  These legs search once and cap that list: nothing deepens, so a list whose cap strikes more
        than depth - top_k entries comes back shorter than top_k.  (Not Mi355Index.collapse_fetch_k: its default, top_k, was
        chosen for the search form, which refills what the cap strikes; here it could only ever shorten the plain top-k.)"""
        if source_fetch_k is not None:
            return int(source_fetch_k)
        return max(int(top_k), min(LIST_SOURCE_FETCH_MULT * int(top_k), 1024))

    @staticmethod
    def _cap_lists(u: _UnitIndex, leg: str, ix: Any, dist: np.ndarray, rows: np.ndarray, per_source: int, source_of: Any,
                   top_k: int) -> tuple[np.ndarray, np.ndarray]:
        """At most `per_source` entries per source in the lists a leg's search returned (Mi355Index.collapse_lists over the
        leg's device key table): [B, top_k] in the lists' order.  The distances are taken from `dist` through the kept
        entries' positions, so a MaxSim leg's fp32 values keep their bits."""
        handle = ix if hasattr(ix, "collapse_lists") else ix.index   # (a ShardedSearcher's lists are global on every rank)
        got = handle.collapse_lists(np.asarray(dist, dtype=np.float64), np.asarray(rows, dtype=np.int64),
                                    u.source_keys(leg, source_of, handle), per_source, top_k, with_keys=False,
                                    with_count=False, with_entries=False)
        out = np.full(got.pos.shape, np.nan, dtype=np.asarray(dist).dtype)
        b, s = np.nonzero(got.pos >= 0)
        out[b, s] = np.asarray(dist)[b, got.pos[b, s]]
        return out, got.ids

    @staticmethod
    def _results_from_block(table: ChunkTable, pos_of_row: np.ndarray, rows: np.ndarray, scores: np.ndarray,
                            with_content: bool) -> list[list[dict]]:
        """[B,k] index rows (-1 padded at the tail) + float64 scores -> the reference's list of result dicts per query.
        Built from whole-array conversions: a page is B*k results, and one Python-level numpy access per result costs
        more than the GPU pass that produced them."""
        k = rows.shape[1]
        neg = rows < 0
        n_valid = np.where(neg.any(axis=1), neg.argmax(axis=1), k).tolist()
        pos = pos_of_row[np.where(neg, 0, rows)].tolist()
        sc = scores.tolist()
        ids, contents = table.ids, table.contents
        if with_content:
            return [[{"doc_id": ids[p], "score": s, "content": contents[p]} for p, s in zip(pr[:n], sr[:n])]
                    for pr, sr, n in zip(pos, sc, n_valid)]
        return [[{"doc_id": ids[p], "score": s, "content": None} for p, s in zip(pr[:n], sr[:n])]
                for pr, sr, n in zip(pos, sc, n_valid)]

    @staticmethod
    def _single_rows_of(u: _UnitIndex, doc_ids: list) -> tuple[list, np.ndarray]:
        """(the keys of `doc_ids` that have a stored single-vector embedding, each once in first-seen order; their index rows)"""
        if u.table.embedding is None:
            return [], np.zeros(0, dtype=np.int64)
        pos, row = u.pos_of_id(), u.stored_row_of_pos()
        known = {pk: row[pos[pk]] for pk in doc_ids if pk in pos and pos[pk] in row}
        return list(known), np.fromiter(known.values(), dtype=np.int64, count=len(known))

    def _single_block(self, Q: np.ndarray, top_k: int, unit: str, within: list | None = None,
                      mmr_fetch_k: int | None = None, mmr_lambda: float = 0.5, per_source: int | None = None,
                      source_of: Any = None, source_fetch_k: int | None = None) -> list[list[dict]]:
        u = self._unit(unit)
        # (one process per GPU, every rank: local top-k of its rows, all-gather, merge -> the same global lists)
        searcher = u.single_searcher(self._world)
        if per_source is not None:
            handle = searcher if hasattr(searcher, "collapse_lists") else searcher.index
            if within is None:   # only the queries whose cap bites are searched deeper (under a _World: on every rank alike)
                got = searcher.search_collapsed(Q, top_k, per_source, u.source_keys("single", source_of, handle), source_fetch_k)
                dist, rows = got.dist, got.rows
            else:
                depth = self._source_depth(top_k, source_fetch_k)
                dist, rows = searcher.search_subset(Q, depth, self._single_rows_of(u, within)[1])
                dist, rows = self._cap_lists(u, "single", searcher, dist, rows, per_source, source_of, top_k)
        elif mmr_fetch_k is not None:
            if within is None:
                dist, rows = searcher.search_mmr(Q, top_k, mmr_fetch_k, mmr_lambda)
            else:   # the mmr_fetch_k nearest of the listed rows are each query's pool (-1 padding is skipped by the library)
                if mmr_fetch_k < top_k:
                    raise ValueError("mmr_fetch_k must be >= top_k")  # noqa: TRY003
                pool = searcher.search_subset(Q, mmr_fetch_k, self._single_rows_of(u, within)[1])[1]
                dist, rows = searcher.mmr_select(Q, top_k, pool, mmr_lambda)
        elif within is None:
            dist, rows = searcher.search(Q, top_k)
        else:   # ... among the listed rows: every rank passes the whole list, the library keeps what falls in its shard
            dist, rows = searcher.search_subset(Q, top_k, self._single_rows_of(u, within)[1])
        # reference: score = 1 - distance (retrieval_pipeline.py:522-524) in Python float arithmetic = IEEE double
        return self._results_from_block(u.table, u.single_rows, rows, 1.0 - dist, unit == "chunk")

    def vector_search_by_embedding(self, embedding: list[float], top_k: int = 10, unit: str = "chunk",
                                   within: list | None = None, mmr_fetch_k: int | None = None,
                                   mmr_lambda: float = 0.5, per_source: int | None = None, source_of: Any = None,
                                   source_fetch_k: int | None = None) -> list[dict]:
        self._check_mmr("single", mmr_fetch_k)
        self._check_per_source(top_k, per_source, source_of, source_fetch_k, mmr_fetch_k)
        if len(embedding) == 0:  # reference: `if not query_vector: return []` (base.py:403-404)
            return []
        return self._single_block(np.asarray(embedding, dtype=np.float32)[None, :], top_k, unit, within, mmr_fetch_k, mmr_lambda,
                                  per_source, source_of, source_fetch_k)[0]

    # ---- range search: everything within a distance, and how many (not in the reference's service) ----
    def _range_block(self, Q: np.ndarray, max_distance, limit: int, unit: str) -> list[tuple[list[dict], int]]:
        """`_single_block` for `WHERE distance <= max_distance ORDER BY distance LIMIT limit`: the same row map and score
        conversion; with every result list the exact number of chunks within the distance (it may exceed `limit`)."""
        if self._world is not None:
            raise NotImplementedError("range search under a process group: the shards' counts and lists are not merged yet")
        u = self._unit(unit)
        dist, rows, count = u.single_searcher(None).search_range(Q, max_distance, limit)
        block = self._results_from_block(u.table, u.single_rows, rows, 1.0 - dist, unit == "chunk")
        return [(res, int(c)) for res, c in zip(block, count.tolist())]

    def vector_search_range_by_embedding(self, embedding: list[float], max_distance: float, limit: int = 10,
                                         unit: str = "chunk") -> tuple[list[dict], int]:
        """(the up to `limit` nearest chunks with cosine distance <= max_distance -- the result dicts and scores of
        `vector_search_by_embedding` --, the number of chunks within that distance)."""
        if len(embedding) == 0:  # (as `vector_search_by_embedding`)
            return [], 0
        return self._range_block(np.asarray(embedding, dtype=np.float32)[None, :], float(max_distance), limit, unit)[0]

    def vector_search_range(self, query_ids: list[int | str], max_distance, limit: int = 10,
                            unit: str = "chunk") -> list[tuple[list[dict], int]]:
        """`vector_search_range_by_embedding` for every stored query id, scored as one block; `max_distance` is a scalar or
        one value per query.  Raises ValueError for an unknown query or one without an embedding, like `vector_search`."""
        queries = []
        for qid, q in zip(query_ids, self.get_queries(list(query_ids)), strict=True):
            if q is None:
                raise ValueError(f"Query {qid} not found")  # noqa: TRY003
            if q.embedding is None:
                msg = f"Query {qid} has no embedding" if unit == "chunk" else f"Query {qid} has no single-vector embedding"
                raise ValueError(msg)
            queries.append(q)
        if not queries:
            return []
        Q = np.stack([q.embedding for q in queries]).astype(np.float32, copy=False)
        return self._range_block(Q, max_distance, limit, unit)

    # ---- search by stored chunk: "more like this" from a primary key (not in the reference's service) ----
    def similar_chunks(self, doc_ids: list, top_k: int = 10, unit: str = "chunk", max_distance=None) -> list:
        """For every key of `doc_ids` the `top_k` nearest OTHER chunks: the result dicts and scores of
        `vector_search_by_embedding` on the chunk's stored embedding, the chunk itself absent.  The stored vectors are read on
        the device.  With `max_distance` (a scalar or one value per key) every entry is (the up to `top_k` nearest other chunks
        within that cosine distance, their exact number), as `vector_search_range` returns.  Raises ValueError for a key
        unknown to the table or without a stored embedding, NotImplementedError under a process group."""
        if self._world is not None:  # (every rank alike, before any collective)
            raise NotImplementedError("similar_chunks under a process group: the query row lives on one shard only")
        doc_ids = list(doc_ids)
        if not doc_ids:
            return []
        u = self._unit(unit)
        row_of = dict(zip(*self._single_rows_of(u, doc_ids)))
        pos = u.pos_of_id()
        for pk in doc_ids:
            if pk not in pos:
                raise ValueError(f"Chunk {pk} not found")  # noqa: TRY003
            if pk not in row_of:
                msg = f"Chunk {pk} has no embedding" if unit == "chunk" else f"Chunk {pk} has no single-vector embedding"
                raise ValueError(msg)
        ids = np.fromiter((row_of[pk] for pk in doc_ids), dtype=np.int64, count=len(doc_ids))
        searcher = u.single_searcher(None)
        if max_distance is None:
            dist, rows = searcher.search_rows(ids, top_k)
            return self._results_from_block(u.table, u.single_rows, rows, 1.0 - dist, unit == "chunk")
        dist, rows, count = searcher.search_range_rows(ids, max_distance, top_k)
        block = self._results_from_block(u.table, u.single_rows, rows, 1.0 - dist, unit == "chunk")
        return [(res, int(c)) for res, c in zip(block, count.tolist())]

    # ---- search by examples and Rocchio feedback: queries built on the device (not in the reference's service) ----
    def _example_rows(self, u: _UnitIndex, doc_ids: list, unit: str) -> np.ndarray:
        """the index rows of the listed keys, in list order; ValueError for an unknown key or one without an embedding"""
        row_of = dict(zip(*self._single_rows_of(u, doc_ids)))
        pos = u.pos_of_id()
        for pk in doc_ids:
            if pk not in pos:
                raise ValueError(f"Chunk {pk} not found")  # noqa: TRY003
            if pk not in row_of:
                msg = f"Chunk {pk} has no embedding" if unit == "chunk" else f"Chunk {pk} has no single-vector embedding"
                raise ValueError(msg)
        return np.fromiter((row_of[pk] for pk in doc_ids), dtype=np.int64, count=len(doc_ids))

    def similar_to_examples(self, positive_ids: list, negative_ids: list = (), top_k: int = 10, unit: str = "chunk",
                            embedding: list[float] | None = None, alpha: float = 1.0, beta: float = 1.0,
                            gamma: float = 1.0, keep: bool = False) -> list[dict]:
        """"More like these, less like those": the `top_k` chunks nearest to alpha * embedding + beta * mean(positives) -
        gamma * mean(negatives) (unit-normalised terms; `embedding` optional), the listed chunks themselves absent unless
        `keep`.  The stored vectors are combined and searched on the device (Mi355Index.search_examples).  Result dicts and
        scores as `vector_search_by_embedding`.  Raises ValueError for a key unknown to the table or without a stored
        embedding, NotImplementedError under a process group."""
        if self._world is not None:  # (every rank alike, before any collective)
            raise NotImplementedError("similar_to_examples under a process group: the examples live on different shards")
        positive_ids, negative_ids = list(positive_ids), list(negative_ids)
        if not positive_ids and (embedding is None or len(embedding) == 0):
            return []
        u = self._unit(unit)
        pos = self._example_rows(u, positive_ids, unit)
        neg = self._example_rows(u, negative_ids, unit)
        base = None if embedding is None or len(embedding) == 0 else np.asarray(embedding, dtype=np.float32)[None, :]
        dist, rows = u.single_searcher(None).search_examples(pos[None, :], top_k, neg_ids=neg[None, :], queries=base,
                                                             alpha=alpha, beta=beta, gamma=gamma, keep=keep)
        return self._results_from_block(u.table, u.single_rows, rows, 1.0 - dist, unit == "chunk")[0]

    def _feedback_block(self, Q: np.ndarray, top_k: int, fb_k: int, alpha: float, beta: float, unit: str) -> list[list[dict]]:
        if self._world is not None:  # (every rank alike, before any collective)
            raise NotImplementedError("feedback search under a process group: the first pass's rows live on different shards")
        u = self._unit(unit)
        dist, rows = u.single_searcher(None).search_feedback(Q, top_k, fb_k, alpha, beta)
        return self._results_from_block(u.table, u.single_rows, rows, 1.0 - dist, unit == "chunk")

    def vector_search_feedback(self, query_ids: list[int | str], top_k: int = 10, fb_k: int = 10, alpha: float = 1.0,
                               beta: float = 0.75, unit: str = "chunk") -> list[list[dict]]:
        """`vector_search` with one round of Rocchio pseudo-relevance feedback, scored as one block: every query is searched
        at `fb_k`, moved to alpha * query + beta * mean(those chunks) (unit-normalised terms) and searched again at `top_k`
        (Mi355Index.search_feedback; the first pass's lists stay on the device).  Raises ValueError for an unknown query or
        one without an embedding, like `vector_search`; NotImplementedError under a process group."""
        if self._world is not None:
            raise NotImplementedError("feedback search under a process group: the first pass's rows live on different shards")
        queries = []
        for qid, q in zip(query_ids, self.get_queries(list(query_ids)), strict=True):
            if q is None:
                raise ValueError(f"Query {qid} not found")  # noqa: TRY003
            if q.embedding is None:
                msg = f"Query {qid} has no embedding" if unit == "chunk" else f"Query {qid} has no single-vector embedding"
                raise ValueError(msg)
            queries.append(q)
        if not queries:
            return []
        Q = np.stack([q.embedding for q in queries]).astype(np.float32, copy=False)
        return self._feedback_block(Q, top_k, fb_k, alpha, beta, unit)

    def vector_search_feedback_by_embedding(self, embedding: list[float], top_k: int = 10, fb_k: int = 10, alpha: float = 1.0,
                                            beta: float = 0.75, unit: str = "chunk") -> list[dict]:
        """`vector_search_feedback` for one embedding."""
        if self._world is not None:
            raise NotImplementedError("feedback search under a process group: the first pass's rows live on different shards")
        if len(embedding) == 0:  # (as `vector_search_by_embedding`)
            return []
        return self._feedback_block(np.asarray(embedding, dtype=np.float32)[None, :], top_k, fb_k, alpha, beta, unit)[0]

    def vector_search_groups(self, embeddings_per_query: list, top_k: int, fetch_k: int | None = None, unit: str = "chunk",
                             search_mode: Literal["single", "multi"] = "single") -> list[list[dict]]:
        """Several searches per question, fused on the device (not in the reference's service: its callers loop in Python,
        e.g. question_decomposition.py:203-220).  `embeddings_per_query[g]` lists the embeddings of question g -- vectors in
        single mode, [n_q, d] matrices in multi mode; every one is searched at `fetch_k` (default top_k) and the lists of a
        question become one: every chunk once, at its best score, the best `top_k` of them.  One result list per question,
        in the reference's order (-score, str(doc_id)).
        single: Mi355Index.search_groups; score = 1.0 - distance, as `_single_block` computes it.
        multi: one `search_maxsim` over all sub-queries, then Mi355Index.merge_groups over val = -(-distance / n_q) in
        float64 -- sub-queries differ in token count, so scores are merged, not distances; score = -val is bit for bit what
        `maxsim_search_by_embeddings` reports.
        Documented difference: the cut at `top_k` is made by (distance, index row) in single mode and (-score, document row)
        in multi mode, so an exact score tie that straddles the cut may keep another member of the tie than the reference's
        (-score, str(doc_id)) order would."""
        fetch_k = int(top_k if fetch_k is None else fetch_k)
        u = self._unit(unit)
        out: list[list[dict]] = [[] for _ in embeddings_per_query]
        if search_mode == "multi":
            ix = u.multi_searcher(self._world)
            dim = u.table.mv_tokens.shape[1]
            mats, sizes = [], []
            for embs in embeddings_per_query:
                ms = [m for m in (np.asarray(e, dtype=np.float32).reshape(-1, dim) for e in embs) if m.shape[0] > 0]
                mats.extend(ms)   # (no query vectors: no results -- `maxsim_search_by_embeddings`)
                sizes.append(len(ms))
            if not mats:
                return out
            lens = np.asarray([m.shape[0] for m in mats], dtype=np.int64)
            qoff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            dist, rows = ix.search_maxsim(np.concatenate(mats, axis=0), qoff, fetch_k)
            vals = -(-np.asarray(dist).astype(np.float64) / lens[:, None])
            merger = ix if hasattr(ix, "merge_groups") else ix.index   # (a ShardedSearcher's lists are global on every rank)
            vals, rows, _ = merger.merge_groups(vals, np.asarray(rows, dtype=np.int64), self._offsets_of(sizes), top_k)
            scores, pos_of_row = -vals, u.multi_rows
        else:
            searcher = u.single_searcher(self._world)
            sizes = [len(embs) for embs in embeddings_per_query]
            if sum(sizes) == 0:
                return out
            Q = np.stack([np.asarray(e, dtype=np.float32) for embs in embeddings_per_query for e in embs])
            dist, rows, _ = searcher.search_groups(Q, self._offsets_of(sizes), top_k, fetch_k)
            scores, pos_of_row = 1.0 - dist, u.single_rows
        block = self._results_from_block(u.table, pos_of_row, rows, scores, unit == "chunk")
        return [sorted(res, key=lambda r: (-r["score"], str(r["doc_id"]))) for res in block]

    @staticmethod
    def _offsets_of(sizes: list[int]) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)

    def score_candidates(self, embedding: list[float], doc_ids: list, unit: str = "chunk") -> dict:
        """Dense score of explicit candidates: {doc_id: 1.0 - cosine distance}, the score `vector_search_by_embedding` gives
        the same chunk (Python float arithmetic).  Ids unknown to the table or without a stored embedding are left out (as
        `maxsim_score_candidates` does); no embedding -> {}."""
        if len(embedding) == 0:
            return {}
        u = self._unit(unit)
        searcher = u.single_searcher(self._world)
        known, rows = self._single_rows_of(u, doc_ids)
        if not known:
            return {}
        dist = searcher.score_subset(np.asarray(embedding, dtype=np.float32)[None, :], rows[None, :])[0]
        return {pk: 1.0 - float(dv) for pk, dv in zip(known, dist)}

    def maxsim_search_by_embeddings(self, query_vectors: list, top_k: int, unit: str = "chunk",
                                    within: list | None = None, per_source: int | None = None, source_of: Any = None,
                                    source_fetch_k: int | None = None) -> list[list[dict]]:
        """`per_source` / `source_of` / `source_fetch_k` (None = today's behaviour): ONE MaxSim search at `source_fetch_k`
        (default LIST_SOURCE_FETCH_MULT * top_k), then at most `per_source` results per source: nothing deepens, a list can
        come back shorter than top_k (`vector_search`)."""
        self._check_per_source(top_k, per_source, source_of, source_fetch_k, None)
        u = self._unit(unit)
        ix = u.multi_searcher(self._world)
        dim = u.table.mv_tokens.shape[1]
        mats = [np.asarray(qv, dtype=np.float32).reshape(-1, dim) for qv in query_vectors]
        lens = [m.shape[0] for m in mats]
        live = [i for i, n in enumerate(lens) if n > 0]
        out: list[list[dict]] = [[] for _ in mats]  # reference: `if not query_vectors: return []`
        if not live:
            return out
        qtok = np.concatenate([mats[i] for i in live], axis=0)
        qoff = np.concatenate([[0], np.cumsum([lens[i] for i in live])]).astype(np.int32)
        depth = top_k if per_source is None else self._source_depth(top_k, source_fetch_k)
        if within is None:
            dist, rows = ix.search_maxsim(qtok, qoff, depth)
        else:
            dist, rows = self._maxsim_within(u, ix, qtok, qoff, depth, within)
        if per_source is not None:
            dist, rows = self._cap_lists(u, "multi", ix, dist, rows, per_source, source_of, top_k)
        # reference: score = -distance / n_query_vectors (retrieval_pipeline.py:511-514): float(f32) negated, divided
        n_q = np.maximum(1, np.asarray([lens[i] for i in live], dtype=np.int64))[:, None]
        scores = -dist.astype(np.float64) / n_q
        for i, res in zip(live, self._results_from_block(u.table, u.multi_rows, rows, scores, unit == "chunk")):
            out[i] = res
        return out

    @staticmethod
    def _maxsim_within(u: _UnitIndex, ix: Any, qtok: np.ndarray, qoff: np.ndarray, top_k: int, within: list):
        """`search_maxsim` among the listed keys.  One `search_maxsim_subset` call where the searcher has it: the list is
        screened and the top-k selected on the device (under a _World each rank the documents it owns, one all-gather of the
        [2, B, k] block).  A searcher without it scores every candidate exactly for every query (maxsim_subset) and the host
        orders them by (distance, document): the same (distance, document) lists."""
        pos, off = u.pos_of_id(), u.table.mv_offsets
        docs = np.array(sorted({pos[pk] for pk in within if pk in pos and off[pos[pk] + 1] > off[pos[pk]]}), dtype=np.int64)
        B = qoff.shape[0] - 1
        dist = np.full((B, top_k), np.nan, dtype=np.float32)
        rows = np.full((B, top_k), -1, dtype=np.int64)
        if docs.size and hasattr(ix, "search_maxsim_subset"):
            d, r = ix.search_maxsim_subset(qtok, qoff, top_k, docs)
            d, r = np.asarray(d, dtype=np.float32), np.asarray(r, dtype=np.int64)
            keep = ~np.isnan(d)   # (an undefined distance is no result, as below)
            dist[keep], rows[keep] = d[keep], r[keep]
        elif docs.size:
            scored = np.asarray(ix.maxsim_subset(qtok, qoff, np.tile(docs, (B, 1))), dtype=np.float32)
            for b in range(B):
                live = np.nonzero(~np.isnan(scored[b]))[0]
                best = live[np.lexsort((docs[live], scored[b, live]))[:top_k]]
                dist[b, :best.size], rows[b, :best.size] = scored[b, best], docs[best]
        return dist, rows

    def maxsim_score_candidates(self, query_vectors, doc_ids: list, unit: str = "chunk") -> dict:
        """Late-interaction score of explicit candidates: {doc_id: mean_i max_j <q_i, d_j>} (reference HEAVEN
        `_score_candidates`, heaven.py:244-266).  Ids unknown to the table or without multi-vector embeddings are left
        out (as `_fetch_candidate_multi_embeddings` does, heaven.py:224-241); no query vectors -> every score 0.0."""
        u = self._unit(unit)
        pos, off = u.pos_of_id(), u.table.mv_offsets
        known = [(pk, pos[pk]) for pk in doc_ids if pk in pos and off is not None and off[pos[pk] + 1] > off[pos[pk]]]
        if not known:
            return {}
        q = np.asarray(query_vectors, dtype=np.float32)
        if q.size == 0:
            return {pk: 0.0 for pk, _ in known}
        # one process per GPU: the token-sharded store -- every rank scores the candidates it owns, one all-gather of [1, m] fp32
        q = q.reshape(-1, u.table.mv_tokens.shape[1])
        rows = np.array([[p for _, p in known]], dtype=np.int64)
        dist = u.multi_searcher(self._world).maxsim_subset(q, np.array([0, q.shape[0]], dtype=np.int32), rows)[0]
        return {pk: -float(dv) / q.shape[0] for (pk, _), dv in zip(known, dist) if dv == dv}

    def maxsim_explain(self, query_vectors, doc_ids: list, unit: str = "chunk", clamp0: bool = False) -> dict:
        """The terms of `maxsim_score_candidates`: {doc_id: {"score", "token_scores": [n_q], "token_matches": [n_q]}} -- per
        query vector its best dot over the document's tokens and the index of the token that gave it (the lowest on a tie;
        ColBERT's token alignment).  Id hygiene and `score` are those of `maxsim_score_candidates` (with `clamp0` every
        vector contributes max(0, .), the ColBERT reranker's form); no query vectors -> {}."""
        u = self._unit(unit)
        pos, off = u.pos_of_id(), u.table.mv_offsets
        known = [(pk, pos[pk]) for pk in doc_ids if pk in pos and off is not None and off[pos[pk] + 1] > off[pos[pk]]]
        q = np.asarray(query_vectors, dtype=np.float32)
        if not known or q.size == 0:
            return {}
        q = q.reshape(-1, u.table.mv_tokens.shape[1])
        rows = np.array([[p for _, p in known]], dtype=np.int64)
        al = u.multi_searcher(self._world).maxsim_align(q, np.array([0, q.shape[0]], dtype=np.int32), rows, clamp0=clamp0)
        return {pk: {"score": -float(al.dist[0, j]) / q.shape[0],
                     "token_scores": np.asarray(al.values[:, j], dtype=np.float32).copy(),
                     "token_matches": np.asarray(al.tokens[:, j], dtype=np.int32).copy()}
                for j, (pk, _) in enumerate(known) if al.dist[0, j] == al.dist[0, j]}

    def maxsim_similarity_map(self, query_vectors, doc_id, unit: str = "chunk") -> np.ndarray | None:
        """Every dot of the query's vectors with the document's tokens: float32 [n_q, T] (ColPali's heat-map over the patches of
        a page).  None for an id unknown to the table or without multi-vector embeddings, and for no query vectors."""
        u = self._unit(unit)
        pos, off = u.pos_of_id(), u.table.mv_offsets
        q = np.asarray(query_vectors, dtype=np.float32)
        if doc_id not in pos or off is None or off[pos[doc_id] + 1] <= off[pos[doc_id]] or q.size == 0:
            return None
        q = q.reshape(-1, u.table.mv_tokens.shape[1])
        return u.multi_searcher(self._world).maxsim_map(q, np.array([0, q.shape[0]], dtype=np.int32), [0], [pos[doc_id]])[0]

    # ---- Guided Query Refinement support (reference retrieval_pipeline.py:573-641 + gqr_hybrid.py:306-362) ----
    def get_query_embedding(self, query_id) -> np.ndarray | None:
        """Stored single-vector query embedding as float64, None when the query or its embedding is missing (:573-587)."""
        q = self.get_queries([query_id])[0]
        return None if q is None or q.embedding is None else np.asarray(q.embedding, dtype=np.float64)

    def get_query_multi_embedding(self, query_id) -> np.ndarray | None:
        """Stored multi-vector query embedding [n_q, d] float64, or None (:589-603)."""
        q = self.get_queries([query_id])[0]
        return None if q is None or q.embeddings is None else np.asarray(q.embeddings, dtype=np.float64)

    def _gqr_handle(self) -> Mi355Index:
        """Any native handle (the score-space refinement needs a device, not an index)."""
        u = self._unit("chunk")
        if u.single is not None or u.multi is not None:
            return u.single if u.single is not None else u.multi
        if getattr(self, "_scratch", None) is None:
            self._scratch = Mi355Index(8, "cosine", self._device)
        return self._scratch

    def chunk_rows_single(self, doc_ids: list) -> np.ndarray | None:
        """Index rows of chunks, or None when one of them has no stored single-vector embedding (the reference's
        `len(embedding_ids) == len(candidate_ids)` test, gqr_hybrid.py:454-456)."""
        u = self._unit("chunk")
        if u.table.embedding is None:
            return None
        if self._world is None:    # (one process per GPU: the mapping only -- the rows are staged per page, see gqr_refine_single)
            u.ensure_single()
        pos, row = u.pos_of_id(), u.stored_row_of_pos()
        rows = [row.get(pos.get(pk, -1), -1) for pk in doc_ids]
        return None if any(r < 0 for r in rows) else np.asarray(rows, dtype=np.int64)

    def chunk_rows_multi(self, doc_ids: list) -> np.ndarray | None:
        """Same for multi-vector embeddings (gqr_hybrid.py:439-441)."""
        u = self._unit("chunk")
        off = u.table.mv_offsets
        if off is None:
            return None
        if self._world is None:
            u.ensure_multi()
        pos = [u.pos_of_id().get(pk, -1) for pk in doc_ids]
        if any(p < 0 or off[p + 1] <= off[p] for p in pos):
            return None
        return np.asarray(pos, dtype=np.int64)

    # The refinement is a loop of n_steps (25) dependent steps over a pool of a few dozen candidates per query: under a
    # _World it is NOT spread over the ranks (a collective per step for a few KB of work).  The pools' vectors -- a page's
    # worth: kilobytes to a few MB -- are staged from the exported table into a scratch store on every rank and refined there,
    # identically on every rank; no rank ever holds the whole table on its GPU for it (reference gqr_hybrid.py:366-406
    # fetches the same vectors out of PostgreSQL per query).
    @staticmethod
    def _compact_pools(pools: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """[B,P] rows (-1 padded) -> (the distinct rows, ascending; the same pools in positions of that list)."""
        pools = np.asarray(pools, dtype=np.int64)
        live = pools >= 0
        uniq, inv = np.unique(pools[live], return_inverse=True)
        local = np.full(pools.shape, -1, dtype=np.int64)
        local[live] = inv
        return uniq, local

    def gqr_refine_single(self, queries: np.ndarray, pools: np.ndarray, comp: np.ndarray, **prm) -> np.ndarray:
        u = self._unit("chunk")
        if self._world is None:
            return u.ensure_single().gqr_refine(queries, pools, comp, **prm)
        uniq, local = self._compact_pools(pools)
        emb = u.table.embedding[u.single_positions()[uniq]]
        with Mi355Index(emb.shape[1], "cosine", self._device) as scratch:
            scratch.add(emb)
            return scratch.gqr_refine(queries, local, comp, **prm)

    def gqr_refine_multi(self, qtok: np.ndarray, q_offsets: np.ndarray, pools: np.ndarray, comp: np.ndarray,
                         **prm) -> np.ndarray:
        u = self._unit("chunk")
        if self._world is None:
            return u.ensure_multi().gqr_refine_maxsim(qtok, q_offsets, pools, comp, **prm)
        uniq, local = self._compact_pools(pools)   # (multi-vector rows are table positions)
        tok, off = u.table.mv_tokens, u.table.mv_offsets
        lens = off[uniq + 1] - off[uniq]
        sub = np.concatenate([tok[off[p]:off[p + 1]] for p in uniq], axis=0) if len(uniq) else tok[:0]
        with Mi355Index(tok.shape[1], "cosine", self._device) as scratch:
            scratch.add_multivec(sub, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
            return scratch.gqr_refine_maxsim(qtok, q_offsets, local, comp, **prm)

    def gqr_refine_scores(self, primary: np.ndarray, counts: np.ndarray, comp: np.ndarray, **prm) -> np.ndarray:
        return self._gqr_handle().gqr_refine_scores(primary, counts, comp, **prm)

    # ---- batch driver (reference _run_pipeline) ----
    @staticmethod
    def _collect_retrieval_results(query_ids, results, pipeline_id, failed_queries, result_id_key) -> list[dict]:
        rows = []
        for qid, res in zip(query_ids, results, strict=True):
            if res is None:
                failed_queries.append(qid)
                continue
            for r in res:
                rows.append({"query_id": qid, "pipeline_id": pipeline_id, result_id_key: r["doc_id"], "rel_score": r["score"]})
        return rows

    def _run_pipeline(self, retrieval_func: RetrievalFunc | None, pipeline_id: int, unit: str, top_k: int = 10,
                      batch_size: int = 128, max_concurrency: int = 16, max_retries: int = 3, retry_delay: float = 1.0,
                      query_limit: int | None = None,
                      block_func: Callable[[list, int], list[list[dict] | None]] | None = None) -> dict[str, Any]:
        """Page through queries, skip completed ones, retrieve, persist; returns the reference's stats dict.

        `retrieval_func` is the reference's per-query coroutine contract (retry with exponential backoff,
        at most `max_concurrency` in flight).  `block_func`, when given, scores a whole page of ids in one
        GPU block instead (results aligned with the ids, None = failed query).
        """
        store = self._store()
        result_id_key = "image_chunk_id" if unit == "image_chunk" else "chunk_id"
        configured = self.from_root(lambda: store.pipeline_config(pipeline_id).get("retrieval_unit", "chunk"))
        if configured == "mixed":
            raise ValueError(f"Pipeline {pipeline_id!r} is configured for mixed results, which cannot be persisted directly.")
        if configured != unit:
            raise ValueError(f"Pipeline {pipeline_id!r} is configured for {configured} results; "
                             f"refusing to persist {unit} results into the same pipeline identity.")

        async def one(qid) -> list[dict] | None:
            assert retrieval_func is not None
            delay = retry_delay
            for attempt in range(max(1, max_retries)):
                res, err = None, None
                try:
                    res = await retrieval_func(qid, top_k)
                except Exception as e:  # noqa: BLE001
                    err = e
                # one process per GPU: an attempt counts only if it succeeded on EVERY rank -- all ranks then retry (or give
                # the query up) together, and their sequences of collective searches stay aligned
                if self.agree(err is None):
                    return res
                if attempt + 1 >= max(1, max_retries):
                    logger.error(f"Retrieval failed for query {qid} after {max_retries} attempts", exc_info=err)
                    return None
                await asyncio.sleep(min(max(delay, retry_delay), 60))
                delay *= 2
            return None

        async def page(qids) -> list[list[dict] | None]:
            sem = asyncio.Semaphore(max(1, max_concurrency))

            async def guarded(q):
                async with sem:
                    return await one(q)

            return list(await asyncio.gather(*[guarded(q) for q in qids]))

        writer = self._world is None or self._world.rank == 0  # one process per GPU: rank 0 reads the page's ids and persists
        if self._world is not None:
            max_concurrency = 1  # the per-query fallback is a sequence of collective searches: the same order on every rank

        def next_page(eff: int, offset: int):
            """(number of queries on the page, ids still to answer) -- (0, []) at the end."""
            queries = store.get_all_queries(limit=eff, offset=offset)
            if not queries:
                return 0, []
            ids = [q.id for q in queries]
            done = store.completed_query_ids(unit, pipeline_id, ids)
            return len(queries), [q for q in ids if q not in done]

        total_queries = total_results = offset = 0
        failed: list = []
        while True:
            if query_limit is not None and total_queries >= query_limit:
                break
            eff = min(batch_size, query_limit - total_queries) if query_limit is not None else batch_size
            n_page, qids = self.from_root(lambda: next_page(eff, offset))
            if n_page == 0:
                break
            if not qids:
                offset += batch_size
                continue
            if block_func is not None:
                results, block_err = None, None
                try:
                    results = block_func(qids, top_k)
                except Exception as e:  # noqa: BLE001
                    block_err = e
                # (one process per GPU: the page is answered as a block only if every rank's block succeeded.  LIMIT of this
                # agreement: it reconciles failures that happen OUTSIDE a collective.  A rank that dies, or raises from a
                # rank-local HIP / out-of-memory error, while its peers are already inside the block's all-gather leaves them
                # blocked there -- what ends that is the process group's own timeout (`init_process_group(timeout=...)`,
                # torchrun's failure detection), not this code; INTEGRATION.md "one process per GPU" says so.)
                if not self.agree(block_err is None):
                    # one bad query (missing / malformed embedding, too many query vectors for a block, an embedding-batch
                    # error) must not abort the run: the page falls back to the reference's per-query path, where retries,
                    # backoff and `failed_queries` apply to that query alone (retrieval_pipeline.py:222-236)
                    logger.error(f"block retrieval failed for a page of {len(qids)} queries; retrying it query by query",
                                 exc_info=block_err)
                    if retrieval_func is None:
                        raise block_err if block_err is not None else RuntimeError("block retrieval failed on another rank")
                    results = asyncio.run(page(qids))
            else:
                results = asyncio.run(page(qids))
            insert_page = getattr(store, "insert_page", None)
            if not writer:  # (the same lists on every rank: count what rank 0 stores)
                failed.extend(q for q, r in zip(qids, results, strict=True) if r is None)
                total_results += sum(len(r) for r in results if r is not None)
            elif callable(insert_page):
                # a store that takes a page as it is (ranked lists per query): skips flattening it into one dict per
                # result row only to regroup them by query again
                failed.extend(q for q, r in zip(qids, results, strict=True) if r is None)
                total_results += insert_page(unit, pipeline_id, qids, results)
            else:
                rows = self._collect_retrieval_results(qids, results, pipeline_id, failed, result_id_key)
                if rows:
                    store.bulk_insert(unit, rows)
                    total_results += len(rows)
            total_queries += len([r for r in results if r is not None])
            offset += n_page
            logger.info(f"Processed {total_queries} queries, stored {total_results} results")
        if failed:
            logger.warning(f"Failed to process {len(failed)} queries after retries: {failed}")
        return {"pipeline_id": pipeline_id, "total_queries": total_queries, "total_results": total_results,
                "failed_queries": failed}

    def run_pipeline(self, retrieval_func: RetrievalFunc, pipeline_id: int, **kw) -> dict[str, Any]:
        return self._run_pipeline(retrieval_func, pipeline_id, "chunk", **kw)

    def run_image_pipeline(self, retrieval_func: RetrievalFunc, pipeline_id: int, **kw) -> dict[str, Any]:
        return self._run_pipeline(retrieval_func, pipeline_id, "image_chunk", **kw)
