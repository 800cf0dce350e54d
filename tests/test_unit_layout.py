"""CPU: the layout of a unit's single-vector index (`service._UnitIndex.single_rows`: index row -> table position) and every
transition between its states, one case per transition.

Each case pins what `refresh` / `compact_single` return, the exact calls the stand-in index (`MutableOracleIndex` of
tests/helpers.py) receives, `single_rows` and `compacted` afterwards, and that the unit answers like one built fresh from the
new table -- the same (primary key, distance bits) lists."""

import numpy as np
import pytest

from autorag_research_amd import service as svc
from helpers import MutableOracleIndex, unit_answers as answers, unit_base as base, unit_built as built, unit_fresh as fresh
from helpers import unit_table as table

NULLS = (4, 5, 33)
NOT_NULL = np.setdiff1d(np.arange(60), NULLS)
COMPACTED = [dict(nulls=(0, 1)), "compact"]     # (from a unit built without NULLs: 58 slots, for the positions 2 .. 59)

# A step is "compact" (`compact_single`) or a newer export (`changed`).  Per case: the NULLs the unit is built over, the steps
# that lead to the state before, the steps under test, what they return, the calls they issue, `single_rows` and `compacted` after
CASES = {
    "over NULLs: an identical export": (NULLS, [], [{}], ["unchanged"], [], NOT_NULL, False),
    "over NULLs: one changed row": (NULLS, [], [dict(vectors={10: 11})], ["relayout"],
                                    [("add", 60), ("remove", [4, 5, 33])], np.arange(60), False),
    "over NULLs: one appended key": (NULLS, [], [dict(appended=1)], ["relayout"],
                                     [("add", 61), ("remove", [4, 5, 33])], np.arange(61), False),
    "over NULLs: nothing to compact": (NULLS, [], ["compact"], [False], [], NOT_NULL, False),
    "no NULLs: two rows become NULL, then compact": ((), [], COMPACTED, ["incremental", True],
                                                     [("remove", [0, 1]), ("compact",)], np.arange(2, 60), True),
    "compacted: a row becomes NULL": ((), COMPACTED, [dict(nulls=(7,))], ["incremental"], [("remove", [5])], np.arange(2, 60), True),
    "compacted: a NULL that kept its slot gets a vector": ((), COMPACTED + [dict(nulls=(7,))], [dict(vectors={7: 8})],
                                                           ["incremental"], [("update", [5])], np.arange(2, 60), True),
    "compacted: a NULL without a slot gets a vector": ((), COMPACTED + [dict(nulls=(7,)), dict(vectors={7: 8})],
                                                       [dict(vectors={0: 2})], ["relayout"], [("add", 60), ("remove", [1])],
                                                       np.arange(60), False),
    "one slot per position: every kind of change in one export": (
        NULLS, [dict(vectors={10: 11})], [dict(vectors={4: 3}, nulls=(20,), appended=1)], ["incremental"],
        [("remove", [20]), ("update", [4]), ("add", 1)], np.arange(61), False),
}


@pytest.fixture(autouse=True)
def stand_in(monkeypatch, oracle):
    monkeypatch.setattr(svc, "Mi355Index", MutableOracleIndex)
    MutableOracleIndex.created = 0


def changed(t, vectors=None, nulls=(), appended=0):
    """`t` with position p holding twice the vector of position q for every p: q of `vectors`, the embeddings of `nulls` NULL
    and `appended` new keys at the end"""
    emb = t.embedding.copy()
    for p, q in (vectors or {}).items():
        emb[p] = t.embedding[q] * 2
    emb[list(nulls)] = np.nan
    more = np.array([emb[50 + i] * np.float32(0.5) + emb[40] for i in range(appended)], np.float32).reshape(appended, emb.shape[1])
    return table(t.ids + [f"new{i}" for i in range(appended)], np.concatenate([emb, more]))


def take(u, t, step):
    if step == "compact":
        return u.compact_single(), t
    t = changed(t, **step)
    return u.refresh(t), t


@pytest.mark.parametrize("nulls, before, steps, outcomes, calls, rows, compacted", list(CASES.values()), ids=list(CASES))
def test_transition(nulls, before, steps, outcomes, calls, rows, compacted):
    t, Q = base(nulls=nulls)
    u = built(t, Q)
    for step in before:
        _, t = take(u, t, step)
    u.single.calls.clear()
    index, created, got = u.single, MutableOracleIndex.created, []
    for step in steps:
        out, t = take(u, t, step)
        got.append(out)
    assert got == outcomes
    assert u.single.calls == calls
    assert np.array_equal(u.single_rows, rows) and len(u.single) == len(rows) and u.compacted is compacted and u.table is t
    relaid = "relayout" in outcomes                 # the only transition that replaces the index
    assert index.closed == relaid and (u.single is not index) == relaid and MutableOracleIndex.created == created + relaid
    assert answers(u, Q) == fresh(t, Q)


def test_nothing_built_defers_and_creates_no_index():
    t0, Q = base(nulls=NULLS)
    u = svc._UnitIndex(t0, 0)
    t1 = changed(t0, {10: 11}, appended=1)
    assert u.refresh(t1) == "deferred"
    assert MutableOracleIndex.created == 0 and u.single is None and u.single_rows is None and u.table is t1
    assert answers(u, Q) == fresh(t1, Q)
