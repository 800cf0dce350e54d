"""CPU: the host layers of "MaxSim explained" over a host stand-in built on the reference (tests/maxsim_align_ref.py) -- the
binding of the three symbols, ShardedSearcher's merge rule at world 1 and under a fake world of two uneven shards, and the
service's two methods (id hygiene, score == maxsim_score_candidates, the empty cases)."""

import ctypes
import threading

import numpy as np
import pytest

import maxsim_align_ref as ref
from helpers import build_golden_stores

F32 = np.float32


def test_the_three_symbols_are_bound_with_their_prototypes(native_built):
    from autorag_research_amd import _native

    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    f32p, i32p, i64p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    want = {"mi355dr_multivec_token_counts": [vp, i64p, i64, i32p],
            "mi355dr_maxsim_align": [vp, f32p, i32p, ci, i64p, ci, ci, f32p, i32p, f32p],
            "mi355dr_maxsim_map": [vp, f32p, i32p, ci, i32p, i64p, i64, i64p, f32p]}
    L = _native.load()
    for name, args in want.items():
        assert name in _native.ABI_SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is ci and list(fn.argtypes) == args, name


def test_index_and_searcher_carry_the_methods():
    from autorag_research_amd.index import MaxSimAlignment, Mi355Index
    from autorag_research_amd.service import Mi355RetrievalService
    from autorag_research_amd.sharded import ShardedSearcher

    assert MaxSimAlignment._fields == ("values", "tokens", "dist")
    for cls in (Mi355Index, ShardedSearcher):
        assert all(callable(getattr(cls, n)) for n in ("multivec_token_counts", "maxsim_align", "maxsim_map"))
    assert callable(Mi355RetrievalService.maxsim_explain) and callable(Mi355RetrievalService.maxsim_similarity_map)


# ---- ShardedSearcher: the merge rule ----
class FakeGather:
    """torch.distributed's all_gather_into_tensor for `world` searchers living in threads of one process."""

    def __init__(self, world):
        self.world, self.slots, self.bar = world, [None] * world, threading.Barrier(world)
        self.rank_of = {}

    def is_initialized(self):
        return False

    def all_gather_into_tensor(self, out, mine, group=None):
        import torch

        r = self.rank_of[threading.get_ident()]
        self.slots[r] = mine.clone()
        self.bar.wait()
        out.copy_(torch.cat(self.slots))
        self.bar.wait()   # (nobody overwrites a slot before everybody has read it)


def _corpus(rng, d, lens):
    docs = [rng.standard_normal((t, d)).astype(F32) for t in lens]
    return np.concatenate(docs), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _case(rng, d=8):
    lens = [3, 0, 33, 1, 6, 2, 0, 5]
    tok, off = _corpus(rng, d, lens)
    q = rng.standard_normal((6, d)).astype(F32)
    qoff = np.array([0, 4, 4, 6], dtype=np.int32)   # (the middle query has no vectors)
    ids = np.array([[0, 7, 2, -1, 9], [1, 2, 3, 4, 5], [6, 5, 5, 3, 1]], dtype=np.int64)
    pairs = ([0, 2, 0, 1, 2], [2, 7, 6, 3, 40])
    return tok, off, q, qoff, ids, pairs


def _searcher(lo, hi, tok, off, d, rank, world, gather):
    from autorag_research_amd.sharded import ShardedSearcher

    s = ShardedSearcher(d, "cosine", 0, index_factory=ref.RefStore)
    s.world, s.rank, s._dist, s.force_pipeline = world, rank, gather, True
    s.add_local_multivec(tok[off[lo]:off[hi]], off[lo:hi + 1] - off[lo], lo)
    return s


def _ask(s, q, qoff, ids, pairs):
    return (s.multivec_token_counts([0, 1, 2, 7, 8, -1]), s.maxsim_align(q, qoff, ids), s.maxsim_align(q, qoff, ids, clamp0=True, want_dist=False),
            s.maxsim_map(q, qoff, *pairs))


def _check(got, whole, q, qoff, ids, pairs):
    cnt, al, al_c, maps = got
    assert np.array_equal(cnt, whole.multivec_token_counts([0, 1, 2, 7, 8, -1]))
    ref.same_alignment(al, whole.maxsim_align(q, qoff, ids))
    ref.same_alignment(al_c, whole.maxsim_align(q, qoff, ids, clamp0=True, want_dist=False))
    want = whole.maxsim_map(q, qoff, *pairs)
    assert len(maps) == len(want)
    for a, b in zip(maps, want):
        ref.same_bits(a, b)


@pytest.mark.parametrize("cut", [None, 3, 7])
def test_sharded_merge_equals_one_store(oracle, cut):
    """world 1 through the pipeline (cut = None), and a fake world of two uneven shards: documents [0, cut) and [cut, 8)"""
    rng = np.random.default_rng(5)
    d = 8
    tok, off, q, qoff, ids, pairs = _case(rng, d)
    whole = ref.RefStore(d)
    whole.add_multivec(tok, off)
    bounds = [(0, 8)] if cut is None else [(0, cut), (cut, 8)]
    gather = FakeGather(len(bounds))
    out = [None] * len(bounds)

    def run(r):
        gather.rank_of[threading.get_ident()] = r
        s = _searcher(*bounds[r], tok, off, d, r, len(bounds), gather)
        out[r] = _ask(s, q, qoff, ids, pairs)

    threads = [threading.Thread(target=run, args=(r,)) for r in range(len(bounds))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    for got in out:   # the same answer on every rank
        assert got is not None, "a rank failed"
        _check(got, whole, q, qoff, ids, pairs)


# ---- the service ----
@pytest.fixture()
def svc(monkeypatch, oracle):
    import autorag_research_amd.service as service

    monkeypatch.setattr(service, "Mi355Index", ref.RefStore)
    store, g = build_golden_stores()
    return service.Mi355RetrievalService(lambda: store), g


def test_service_explain_and_map(svc, oracle):
    s, g = svc
    ids = list(g["ids"])
    with_mv = [pk for pk, m in zip(ids, g["multivec"]) if m is not None and len(m)]
    without = [pk for pk, m in zip(ids, g["multivec"]) if m is None or not len(m)]
    q = np.asarray(g["Qm"][1], dtype=F32)
    asked = with_mv[:3] + ["no such id"] + without[:1] + with_mv[:1]
    scores = s.maxsim_score_candidates(q, asked)
    ex = s.maxsim_explain(q, asked)
    assert set(ex) == set(scores) == set(with_mv[:3])          # unknown keys and documents without vectors are left out
    for pk in ex:
        doc = np.asarray(g["multivec"][ids.index(pk)], dtype=F32)
        assert ex[pk]["score"] == scores[pk]                    # exactly the float of maxsim_score_candidates
        dd = ref.dots(q, doc)
        ref.same_bits(ex[pk]["token_scores"], dd.max(axis=1))
        assert np.array_equal(ex[pk]["token_matches"], dd.argmax(axis=1)) and ex[pk]["token_matches"].dtype == np.int32
        ref.same_bits(s.maxsim_similarity_map(q, pk), dd)
    cl = s.maxsim_explain(q, with_mv[:2], clamp0=True)
    for pk in cl:
        assert np.array_equal(cl[pk]["token_scores"], np.maximum(ex[pk]["token_scores"], 0))
        assert np.array_equal(cl[pk]["token_matches"], ex[pk]["token_matches"])
    # the empty cases
    assert s.maxsim_explain(q, []) == {} and s.maxsim_explain(q, ["no such id"]) == {}
    assert s.maxsim_explain(np.zeros((0, q.shape[1]), F32), with_mv[:2]) == {}
    assert s.maxsim_similarity_map(q, "no such id") is None
    assert s.maxsim_similarity_map(np.zeros((0, q.shape[1]), F32), with_mv[0]) is None
    if without:
        assert s.maxsim_similarity_map(q, without[0]) is None
