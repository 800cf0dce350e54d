"""CPU: `service._UnitIndex.refresh` applies the difference between two exports of a table to the live index.

The index is a stand-in over numpy and the CPU oracle (`MutableOracleIndex`) that counts the calls it receives: every case
must answer like a unit built fresh from the new table -- the same (primary key, distance) lists -- and must issue only the
calls the difference needs."""

import numpy as np
import pytest

from autorag_research_amd import service as svc
from autorag_research_amd.store import ChunkTable
from helpers import UNIT_D as D, MutableOracleIndex, unit_answers as answers, unit_base as base, unit_built as built
from helpers import unit_fresh as fresh, unit_table as table


@pytest.fixture(autouse=True)
def stand_in(monkeypatch, oracle):
    monkeypatch.setattr(svc, "Mi355Index", MutableOracleIndex)
    MutableOracleIndex.created = 0


def test_changed_embeddings_are_updated_in_place():
    t0, Q = base()
    u = built(t0, Q)
    emb = t0.embedding.copy()
    emb[[3, 17, 40]] = np.random.default_rng(6).standard_normal((3, D)).astype(np.float32)
    t1 = table(t0.ids, emb)
    assert u.refresh(t1) == "incremental"
    assert u.single.calls == [("update", [3, 17, 40])]
    assert answers(u, Q) == fresh(t1, Q)
    assert MutableOracleIndex.created == 2      # the unit's own + the fresh one: no rebuild
    assert u.refresh(table(t0.ids, emb)) == "unchanged" and u.single.calls == [("update", [3, 17, 40])]


def test_embeddings_set_to_null_are_removed_and_filled_again_by_update():
    t0, Q = base()
    u = built(t0, Q)
    emb = t0.embedding.copy()
    emb[[0, 8, 59]] = np.nan
    t1 = table(t0.ids, emb)
    assert u.refresh(t1) == "incremental"
    assert u.single.calls == [("remove", [0, 8, 59])]
    got = answers(u, Q)
    assert got == fresh(t1, Q)
    assert not {"pk000", "pk008", "pk059"} & {pk for res in got for pk, _ in res}
    # NULL -> vector: the slot is revived by an update; one more row changes and one more goes NULL in the same export
    emb2 = emb.copy()
    emb2[[8, 59]] = np.random.default_rng(7).standard_normal((2, D)).astype(np.float32)
    emb2[20] = emb2[21]
    emb2[30] = np.nan
    t2 = table(t0.ids, emb2)
    u.single.calls.clear()
    assert u.refresh(t2) == "incremental"
    assert u.single.calls == [("remove", [30]), ("update", [8, 20, 59])]
    assert answers(u, Q) == fresh(t2, Q)      # (rows 20 and 21 tie exactly: slots stay in table order, so does the tie-break)
    assert u.single.live_rows == 60 - 2 and len(u.single) == 60


def test_appended_keys_are_added():
    t0, Q = base()
    u = built(t0, Q)
    more = np.random.default_rng(8).standard_normal((5, D)).astype(np.float32)
    more[2] = np.nan                             # a new key whose embedding is still NULL
    t1 = table(t0.ids + [f"new{i}" for i in range(5)], np.concatenate([t0.embedding, more]))
    assert u.refresh(t1) == "incremental"
    assert u.single.calls == [("add", 5), ("remove", [62])]
    assert answers(u, Q) == fresh(t1, Q)
    emb = t1.embedding.copy()
    emb[62] = Q[0]                               # ... filled later: revived in place, and the best answer of query 0
    t2 = table(t1.ids, emb)
    u.single.calls.clear()
    assert u.refresh(t2) == "incremental" and u.single.calls == [("update", [62])]
    got = answers(u, Q)
    assert got == fresh(t2, Q) and got[0][0][0] == "new2"


def test_index_built_over_null_rows_is_laid_out_once_then_follows_in_place():
    t0, Q = base(nulls=(4, 5, 33))
    u = built(t0, Q)
    assert len(u.single) == 57 and not u.slot_per_position      # never refreshed: the compacted NOT NULL order
    emb = t0.embedding.copy()
    emb[5] = np.random.default_rng(9).standard_normal(D).astype(np.float32)
    t1 = table(t0.ids, emb)
    old_index = u.single
    assert u.refresh(t1) == "relayout"
    assert old_index.closed and u.slot_per_position and len(u.single) == 60
    assert u.single.calls == [("add", 60), ("remove", [4, 33])]
    assert answers(u, Q) == fresh(t1, Q)
    emb2 = emb.copy()
    emb2[4] = np.random.default_rng(10).standard_normal(D).astype(np.float32)
    emb2[50] = np.nan
    t2 = table(t0.ids, emb2)
    u.single.calls.clear()
    assert u.refresh(t2) == "incremental"
    assert u.single.calls == [("remove", [50]), ("update", [4])]
    assert answers(u, Q) == fresh(t2, Q)


def test_a_reordered_key_list_triggers_the_rebuild(caplog):
    t0, Q = base()
    u = built(t0, Q)
    first = u.single
    order = list(range(60))
    order[10], order[11] = order[11], order[10]
    t1 = table([t0.ids[i] for i in order], t0.embedding[order])
    with caplog.at_level("INFO", logger="AutoRAG-Research"):
        assert u.refresh(t1) == "rebuild"
    assert "full rebuild" in caplog.text and "order changed" in caplog.text
    assert first.closed and first.calls == [] and u.single is None
    assert answers(u, Q) == fresh(t1, Q)
    assert u.single is not first and u.single.calls == [("add", 60)]
    # a key that disappeared is a changed key list too
    u2 = built(t0, Q)
    assert u2.refresh(table(t0.ids[:-1], t0.embedding[:-1])) == "rebuild"


def test_multi_vector_units_and_unbuilt_units():
    t0, Q = base()
    u = svc._UnitIndex(t0, 0)
    t1 = table(t0.ids, t0.embedding + 1)
    assert u.refresh(t1) == "deferred" and u.table is t1 and MutableOracleIndex.created == 0
    u = built(t0, Q)
    tok = np.ones((60, D), np.float32)
    t2 = ChunkTable(ids=list(t0.ids), contents=list(t0.contents), embedding=t0.embedding, mv_tokens=tok,
                    mv_offsets=np.arange(61, dtype=np.int64))
    assert u.refresh(t2) == "rebuild" and u.single is None


def test_chunk_rows_follow_every_kind_of_refresh():
    """`chunk_rows_single` (key -> index row, for the GQR pools) caches two maps on the unit: both must follow the table.
    The row it names must hold the key's CURRENT vector, and a key whose embedding is NULL has no row (None)."""
    from autorag_research_amd.store import InMemoryStore

    def rows_hold_current_vectors(s, t, keys):
        rows = s.chunk_rows_single(keys)
        u = s._unit("chunk")
        want = np.stack([t.embedding[t.ids.index(pk)] for pk in keys])
        assert np.array_equal(u.single._rows[rows].view(np.uint32), want.view(np.uint32))
        assert u.single._live[rows].all()

    t0, _ = base(nulls=(4, 5, 33))
    store = InMemoryStore()
    store.chunks = t0
    s = svc.Mi355RetrievalService(lambda: store)
    keys = ["pk003", "pk006", "pk040", "pk059"]
    rows_hold_current_vectors(s, t0, keys)
    assert s.chunk_rows_single(["pk003", "pk005"]) is None          # NULL embedding: no stored vector
    s.maxsim_score_candidates([], keys)                             # (another reader of the key map, in between)
    # relayout: compacted rows 3, 4, 38, 56 become slots 3, 6, 40, 59
    emb = t0.embedding.copy()
    emb[5] = np.random.default_rng(11).standard_normal(D).astype(np.float32)
    emb[40] = emb[3] * 2
    t1 = table(t0.ids, emb)
    assert s.refresh_unit("chunk", t1) == "relayout"
    rows_hold_current_vectors(s, t1, keys + ["pk005"])
    assert s.chunk_rows_single(["pk004"]) is None and s.chunk_rows_single(["pk033", "pk003"]) is None
    # incremental: a removed slot still holds a vector, but its key has no stored embedding any more
    emb2 = emb.copy()
    emb2[6] = np.nan
    emb2[4] = emb2[7]
    t2 = table(t0.ids + ["new0"], np.concatenate([emb2, emb2[:1] + 1]))
    assert s.refresh_unit("chunk", t2) == "incremental"
    assert s.chunk_rows_single(["pk006"]) is None and s.chunk_rows_single(keys) is None
    rows_hold_current_vectors(s, t2, ["pk003", "pk004", "pk040", "pk059", "new0"])
    # rebuild: reordered keys, compacted again
    order = list(range(61))[::-1]
    t3 = table([t2.ids[i] for i in order], t2.embedding[order])
    assert s.refresh_unit("chunk", t3) == "rebuild"
    rows_hold_current_vectors(s, t3, ["pk003", "pk004", "pk040", "pk059", "new0"])
    assert s.chunk_rows_single(["pk006"]) is None
    assert s.refresh_unit("image_chunk", t3) == "deferred"          # nothing built for that unit
    s.close()
