"""CPU: `service._UnitIndex.refresh` applies the difference between two exports of a MULTI-VECTOR table to the live store.

The index is a stand-in over numpy and the CPU oracle (`MutableOracleStore`) that counts the calls it receives: every case must
answer like a unit built fresh from the new table -- the same (primary key, distance bits) lists -- and must issue only the calls
the difference needs: one `set_multivec` for the documents that changed, lost or regained their vectors, one `add_multivec` for
the keys appended at the end."""

import numpy as np
import pytest

from autorag_research_amd import service as svc
from autorag_research_amd.store import ChunkTable, InMemoryStore
from helpers import UNIT_D as D, UNIT_K as K, MutableOracleStore, mv_answers as answers, mv_base as base, mv_built as built
from helpers import mv_fresh as fresh, mv_table as table


@pytest.fixture(autouse=True)
def stand_in(monkeypatch, oracle):
    monkeypatch.setattr(svc, "Mi355Index", MutableOracleStore)
    MutableOracleStore.created = 0


def test_changed_lost_revived_and_appended_documents_are_applied_in_place():
    ids, docs, _, Q = base()
    t0 = table(ids, docs)
    u = built(t0, Q)
    rng = np.random.default_rng(16)
    new = list(docs)
    new[3] = rng.standard_normal(docs[3].shape).astype(np.float32)               # re-embedded, the same token count
    new[11] = rng.standard_normal((docs[11].shape[0] + 40, D)).astype(np.float32)  # another token count
    new[12] = new[12].copy()
    new[12][-1, 5] = np.float32(-0.0) if new[12][-1, 5] == 0 else -new[12][-1, 5]  # one value of one token
    new[30] = new[30][:0]                                                        # lost its vectors
    new[7] = rng.standard_normal((9, D)).astype(np.float32)                      # had none: revived
    more = [rng.standard_normal((4, D)).astype(np.float32), np.zeros((0, D), np.float32), rng.standard_normal((33, D)).astype(np.float32)]
    t1 = table(ids + ["new0", "new1", "new2"], new + more)
    store = u.multi
    assert u.refresh(t1) == "incremental"
    assert u.multi is store and not store.closed
    assert store.calls == [("set_multivec", [3, 7, 11, 12, 30], [docs[3].shape[0], 9, docs[11].shape[0] + 40, docs[12].shape[0], 0]),
                           ("add_multivec", 3)]
    got = answers(u, Q)
    assert got == fresh(t1, Q)
    assert MutableOracleStore.created == 2      # the unit's own + the fresh one: no rebuild
    assert not {"pk030", "pk020", "new1"} & {pk for res in got for pk, _ in res}
    assert store.n_docs() == 43 and store.live_docs() == 43 - 3 and np.array_equal(u.multi_rows, np.arange(43))


def test_only_a_set_or_only_an_add_is_issued():
    ids, docs, _, Q = base()
    u = built(table(ids, docs), Q)
    new = list(docs)
    new[0] = new[0][:1]
    t1 = table(ids, new)
    assert u.refresh(t1) == "incremental" and u.multi.calls == [("set_multivec", [0], [1])]
    assert answers(u, Q) == fresh(t1, Q)
    u.multi.calls.clear()
    t2 = table(ids + ["z"], new + [docs[1] * 2])
    assert u.refresh(t2) == "incremental" and u.multi.calls == [("add_multivec", 1)]
    assert answers(u, Q) == fresh(t2, Q)


def test_an_identical_export_is_unchanged():
    ids, docs, _, Q = base()
    t0 = table(ids, docs)
    u = built(t0, Q)
    t1 = table(ids, [t.copy() for t in docs])
    assert u.refresh(t1) == "unchanged" and u.multi.calls == [] and u.table is t1
    assert answers(u, Q) == fresh(t0, Q)


def test_reordered_keys_and_a_changed_width_rebuild():
    ids, docs, _, Q = base()
    t0 = table(ids, docs)
    u = built(t0, Q)
    first = u.multi
    order = list(range(len(ids)))
    order[10], order[11] = order[11], order[10]
    t1 = table([ids[i] for i in order], [docs[i] for i in order])
    assert u.refresh(t1) == "rebuild"
    assert first.closed and first.calls == [] and u.multi is None
    assert answers(u, Q) == fresh(t1, Q) and u.multi is not first
    # another width of the token vectors
    u2 = built(t0, Q)
    wide = table(ids, [np.concatenate([t, t], axis=1) for t in docs], dim=2 * D)
    assert u2.refresh(wide) == "rebuild" and u2.multi is None
    # a key that disappeared
    u3 = built(t0, Q)
    assert u3.refresh(table(ids[:-1], docs[:-1])) == "rebuild"
    # the column disappeared
    u4 = built(t0, Q)
    gone = ChunkTable(ids=list(ids), contents=list(t0.contents), embedding=np.ones((len(ids), D), np.float32))
    assert u4.refresh(gone) == "rebuild"


def test_a_unit_with_both_indexes_takes_both_differences():
    ids, docs, emb, Q = base(with_single=True)
    t0 = table(ids, docs, emb)
    u = svc._UnitIndex(t0, 0)
    answers(u, Q)
    u.ensure_single()
    u.multi.calls.clear(), u.single.calls.clear()
    emb1 = emb.copy()
    emb1[5] = emb1[6]
    new = list(docs)
    new[9] = new[9][::-1].copy()
    t1 = table(ids, new, emb1)
    assert u.refresh(t1) == "incremental"
    assert u.single.calls == [("update", [5])] and u.multi.calls == [("set_multivec", [9], [docs[9].shape[0]])]
    assert answers(u, Q) == fresh(t1, Q)
    # only the single-vector column changes: the multi-vector store is not called
    emb2 = emb1.copy()
    emb2[0] = np.nan
    u.multi.calls.clear(), u.single.calls.clear()
    assert u.refresh(table(ids, new, emb2)) == "incremental"
    assert u.single.calls == [("remove", [0])] and u.multi.calls == []
    assert u.refresh(table(ids, new, emb2)) == "unchanged"


def test_chunk_rows_multi_follows_the_refresh():
    ids, docs, _, Q = base()
    store = InMemoryStore()
    store.chunks = table(ids, docs)
    s = svc.Mi355RetrievalService(lambda: store)
    assert s.chunk_rows_multi(["pk003", "pk030"]).tolist() == [3, 30]
    assert s.chunk_rows_multi(["pk003", "pk007"]) is None                        # no vectors
    new = list(docs)
    new[30] = new[30][:0]
    new[7] = docs[3][:2]
    t1 = table(ids + ["tail"], new + [docs[4]])
    assert s.refresh_unit("chunk", t1) == "incremental"
    assert s.chunk_rows_multi(["pk003", "pk030"]) is None
    assert s.chunk_rows_multi(["pk007", "tail"]).tolist() == [7, 40]
    assert s._unit("chunk").multi.calls[-2:] == [("set_multivec", [7, 30], [2, 0]), ("add_multivec", 1)]
    s.close()


def test_only_the_multi_vector_index_built_forgets_the_old_null_pattern():
    """`single_positions()` caches the NOT NULL positions of the table it was asked about; a refresh that only the multi-vector
    index follows must not leave that answer standing over the new table, and "unchanged" means neither column changed."""
    ids, docs, emb, Q = base(with_single=True)
    emb[4] = np.nan
    u = built(table(ids, docs, emb), Q)
    assert u.single is None and 4 not in u.single_positions()
    emb1 = emb.copy()
    emb1[4], emb1[9] = emb[5], np.nan                                            # one NULL filled, another row became NULL
    new = list(docs)
    new[2] = new[2][:3]
    assert u.refresh(table(ids, new, emb1)) == "incremental" and u.multi.calls == [("set_multivec", [2], [3])]
    pos = u.single_positions()
    assert 4 in pos and 9 not in pos and pos.shape[0] == len(ids) - 1
    # the embedding column alone changed: nothing to apply, but not "unchanged" either, and the positions follow again
    emb2 = emb1.copy()
    emb2[9] = emb[9]
    u.multi.calls.clear()
    assert u.refresh(table(ids, new, emb2)) == "incremental" and u.multi.calls == []
    assert u.single_positions().shape[0] == len(ids)
    assert u.refresh(table(ids, new, emb2.copy())) == "unchanged"
    assert u.single_positions().shape[0] == len(ids)


def single_answers(unit, queries, k=K):
    """[(primary key, distance bits)] per query, through the unit's index row -> table position mapping"""
    dist, rows = unit.ensure_single().search(queries, k)
    return [[(unit.table.ids[unit.single_rows[r]], np.float32(x).view(np.uint32)) for x, r in zip(dr, rr) if r >= 0]
            for dr, rr in zip(dist, rows)]


def test_a_multi_only_change_leaves_a_compacted_single_vector_index_alone():
    """Both indexes built over a table with a NULL embedding: the single-vector index holds the NOT NULL rows compacted.  A
    refresh in which only a multi-vector document changed must not touch its rows -> positions map; a later change of the
    embedding column then lays it out with one slot per position as usual."""
    ids, docs, emb, Q = base(with_single=True)
    emb[4] = np.nan
    t0 = table(ids, docs, emb)
    u = svc._UnitIndex(t0, 0)
    answers(u, Q)
    queries = np.random.default_rng(17).standard_normal((5, D)).astype(np.float32)
    before = single_answers(u, queries)
    assert len(u.single) == len(ids) - 1 and u.single_rows.tolist() == [i for i in range(len(ids)) if i != 4]
    u.multi.calls.clear(), u.single.calls.clear()
    new = list(docs)
    new[9] = new[9][::-1][:-1].copy()
    t1 = table(ids, new, emb.copy())
    assert u.refresh(t1) == "incremental"
    assert u.single.calls == [] and u.multi.calls == [("set_multivec", [9], [docs[9].shape[0] - 1])]
    assert u.single_rows.tolist() == [i for i in range(len(ids)) if i != 4] and not u.slot_per_position
    assert single_answers(u, queries) == before == single_answers(svc._UnitIndex(t1, 0), queries)
    assert answers(u, Q) == fresh(t1, Q)
    # now both columns change: the compacted index is laid out anew once, the store takes its set
    emb2 = emb.copy()
    emb2[4], emb2[6] = emb[5], np.nan
    new2 = list(new)
    new2[0] = new2[0][:2]
    t2 = table(ids, new2, emb2)
    assert u.refresh(t2) == "relayout" and u.slot_per_position
    assert single_answers(u, queries) == single_answers(svc._UnitIndex(t2, 0), queries)
    assert answers(u, Q) == fresh(t2, Q)
