"""CPU: compaction of a unit's single-vector index (`service._UnitIndex.compact_single`, the `compact_dead_fraction` policy of
`refresh`, `Mi355RetrievalService.compact_unit`).

The index is the stand-in of tests/helpers.py over numpy and the CPU oracle, with a `compact()` of Mi355Index's
semantics that records its call: every case must answer like a unit built fresh from the table -- the same (primary key,
distance bits) lists -- and must issue only the calls the difference needs."""

import functools

import numpy as np
import pytest

from autorag_research_amd import service as svc
from helpers import UNIT_D as D, MutableOracleIndex, unit_answers as answers, unit_base, unit_built as built
from helpers import unit_fresh as fresh, unit_table as table

base = functools.partial(unit_base, key="pk{:05d}")


@pytest.fixture(autouse=True)
def stand_in(monkeypatch, oracle):
    monkeypatch.setattr(svc, "Mi355Index", MutableOracleIndex)
    MutableOracleIndex.created = 0


def with_nulls(t, nulls):
    emb = t.embedding.copy()
    emb[list(nulls)] = np.nan
    return table(t.ids, emb)


def test_compact_single_answers_like_a_fresh_unit_with_one_compact():
    t0, Q = base()
    u = built(t0, Q)
    assert not u.compact_single() and u.single.calls == []          # nothing dead: nothing to do
    t1 = with_nulls(t0, (0, 1, 8, 30, 59))
    assert u.refresh(t1) == "incremental"
    first = u.single
    u.single.calls.clear()
    assert u.compact_single()
    assert u.single is first and u.single.calls == [("compact",)]
    assert u.compacted and not u.slot_per_position
    assert len(u.single) == u.single.live_rows == 55
    assert np.array_equal(u.single_rows, np.setdiff1d(np.arange(60), [0, 1, 8, 30, 59]))
    assert answers(u, Q) == fresh(t1, Q)
    assert not u.compact_single() and u.single.calls == [("compact",)]
    assert MutableOracleIndex.created == 2                            # the unit's own + the fresh one


def test_refresh_after_a_compaction_stays_in_place():
    t0, Q = base()
    u = built(t0, Q)
    t1 = with_nulls(t0, (2, 3, 40))
    u.refresh(t1)
    u.compact_single()
    u.single.calls.clear()
    created = MutableOracleIndex.created
    rng = np.random.default_rng(11)
    emb = t1.embedding.copy()
    emb[[0, 10, 50]] = rng.standard_normal((3, D)).astype(np.float32)   # changed (slots 0, 8, 47)
    emb[[5, 59]] = np.nan                                               # nulled (slots 3, 56)
    emb[21] = emb[20]                                                   # an exact tie, in table order
    more = rng.standard_normal((4, D)).astype(np.float32)
    more[1] = np.nan                                                    # a newcomer that is still NULL
    t2 = table(t1.ids + [f"new{i}" for i in range(4)], np.concatenate([emb, more]))
    assert u.refresh(t2) == "incremental"
    assert u.single.calls == [("remove", [3, 56]), ("update", [0, 8, 19, 47]), ("add", 4), ("remove", [58])]
    assert MutableOracleIndex.created == created and u.compacted
    assert answers(u, Q) == fresh(t2, Q)
    # the nulled rows kept their slots: they are revived in place; and an unchanged export stays "unchanged"
    emb3 = t2.embedding.copy()
    emb3[[5, 61]] = rng.standard_normal((2, D)).astype(np.float32)
    t3 = table(t2.ids, emb3)
    u.single.calls.clear()
    assert u.refresh(t3) == "incremental" and u.single.calls == [("update", [3, 58])]
    assert answers(u, Q) == fresh(t3, Q)
    assert u.refresh(table(t3.ids, emb3)) == "unchanged"
    # a second compaction after more removals
    t4 = with_nulls(t3, (0, 63))
    assert u.refresh(t4) == "incremental" and u.compact_single()
    assert answers(u, Q) == fresh(t4, Q) and len(u.single) == u.single.live_rows
    assert MutableOracleIndex.created == created + 3                    # (three fresh units only)


def test_a_null_whose_slot_is_gone_regaining_a_vector_is_a_relayout():
    t0, Q = base()
    u = built(t0, Q)
    t1 = with_nulls(t0, (7, 8))
    u.refresh(t1)
    u.compact_single()
    old_index = u.single
    emb = t1.embedding.copy()
    emb[7] = Q[0]
    t2 = table(t1.ids, emb)
    assert u.refresh(t2) == "relayout"
    assert old_index.closed and not u.compacted and u.slot_per_position and len(u.single) == 60
    assert u.single.calls == [("add", 60), ("remove", [8])]
    got = answers(u, Q)
    assert got == fresh(t2, Q) and got[0][0][0] == "pk00007"
    # ... and from then on the unit follows in place again
    t3 = with_nulls(t2, (20,))
    u.single.calls.clear()
    assert u.refresh(t3) == "incremental" and u.single.calls == [("remove", [20])]


def test_without_the_policy_compact_is_never_called():
    t0, Q = base()
    u = built(t0, Q)
    t1 = with_nulls(t0, range(0, 55))
    assert u.refresh(t1) == "incremental"
    assert ("compact",) not in u.single.calls and len(u.single) == 60 and u.single.live_rows == 5
    assert answers(u, Q) == fresh(t1, Q)


def test_the_dead_fraction_decides():
    # (2 000 rows: more than 1 024 of the head stay live, so only the fraction can ask for a compaction)
    t0, Q = base(n=2000, d=4)
    u = built(t0, Q, compact_dead_fraction=0.25)
    t1 = with_nulls(t0, range(100, 599))                                # 499 of 2 000 dead: below a quarter
    assert u.refresh(t1) == "incremental" and ("compact",) not in u.single.calls
    t2 = with_nulls(t1, (1999,))                                        # 500 of 2 000: the fraction is met
    u.single.calls.clear()
    assert u.refresh(t2) == "compacted"
    assert u.single.calls == [("remove", [1999]), ("compact",)]
    assert len(u.single) == u.single.live_rows == 1500 and u.compacted
    assert answers(u, Q) == fresh(t2, Q)
    # the fraction counts against the compacted size from here on
    t3 = with_nulls(t2, range(0, 100))
    u.single.calls.clear()
    assert u.refresh(t3) == "incremental" and u.single.calls == [("remove", list(range(100)))]
    assert answers(u, Q) == fresh(t3, Q)


def test_a_dead_head_decides():
    t0, Q = base(n=66000, d=4)
    u = built(t0, Q, compact_dead_fraction=0.999)
    t1 = with_nulls(t0, range(0, 64513))                                # 1 023 of the first 65 536 slots stay live
    assert u.refresh(with_nulls(t0, range(0, 64512))) == "incremental"  # 1 024 live: not yet
    assert u.refresh(t1) == "compacted"
    assert u.single.calls[-2:] == [("remove", [64512]), ("compact",)]
    assert len(u.single) == 66000 - 64513
    assert answers(u, Q) == fresh(t1, Q)


def test_the_service_plumbs_the_policy_and_compact_unit_and_gqr_rows_follow():
    from autorag_research_amd.store import InMemoryStore

    t0, Q = base()
    store = InMemoryStore()
    store.chunks = t0
    s = svc.Mi355RetrievalService(lambda: store)
    assert not s.compact_unit("chunk")                                  # no unit yet
    u = s._unit("chunk")
    assert u.compact_dead_fraction is None
    assert np.array_equal(s.chunk_rows_single(["pk00000", "pk00010", "pk00059"]), [0, 10, 59])
    assert not s.compact_unit("chunk")                                  # nothing dead
    t1 = with_nulls(t0, (0, 1, 2))
    assert s.refresh_unit("chunk", t1) == "incremental"
    assert np.array_equal(s.chunk_rows_single(["pk00010", "pk00059"]), [10, 59])
    assert s.compact_unit("chunk") and u.single.calls[-1] == ("compact",)
    assert np.array_equal(s.chunk_rows_single(["pk00003", "pk00010", "pk00059"]), [0, 7, 56])
    assert s.chunk_rows_single(["pk00001"]) is None
    s2 = svc.Mi355RetrievalService(lambda: store, compact_dead_fraction=0.5)
    assert s2._unit("chunk").compact_dead_fraction == 0.5
