"""GPU: the hybrid fusion (mi355dr_fuse_lists / _device, csrc/k_fuse.h) against tests/fuse_ref.py: ids equal, scores equal AS
BITS, counts and NaN / -1 tails equal -- for RRF and the four convex combinations, the host and the device form.

The inputs (fuse_ref.all_inputs) are the smallest at which the kernel can go wrong: widths 1, below / at / around one wave,
the 1024 cap and a lopsided pair; identical, disjoint, half-shared (opposite order) and independent lists; -1 tails of
different lengths, a -1 and a NaN in the middle; an empty list 1, list 2, both; a column of equal scores; a one-entry column;
signed zeros; every score mode; weights 0, 1 and 0.3; maps (identity, a shorter non-identity one with a -1); B of 1, 3 and
1030.  Every input is fused at k_out = 1, the first union's size, and above every union."""

import ctypes

import numpy as np
import pytest

import fuse_ref
from fuse_ref import same

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -4
INPUTS = fuse_ref.all_inputs()
_want: dict = {}


@pytest.fixture(scope="module")
def idx(native_built):
    import autorag_research_amd as pkg

    with pkg.Mi355Index(8) as ix:
        yield ix


def k_top(lists):
    return min(lists[0].shape[1] + lists[2].shape[1] + 3, 2048)


def keywords(lists, kw, method):
    return {**kw, "method": method, "fetch_k": max(lists[0].shape[1], lists[2].shape[1])}


def want_of(i, method):
    """the reference at the largest k_out, computed once per (input, method) and never changed: a smaller k_out is its prefix"""
    if (i, method) not in _want:
        _, lists, kw = INPUTS[i]
        _want[i, method] = fuse_ref.fuse_lists(*lists, k_top(lists), **keywords(lists, kw, method))
    return _want[i, method]


def cut(want, k):
    return want[0][:, :k], want[1][:, :k], want[2]


@pytest.mark.parametrize("method", fuse_ref.METHODS)
def test_host_form_equals_the_reference(idx, method):
    for i, (name, lists, kw) in enumerate(INPUTS):
        want = want_of(i, method)
        for k in sorted({1, max(int(want[2][0]), 1), k_top(lists)}):
            try:
                same(idx.fuse_lists(*lists, k, **keywords(lists, kw, method)), cut(want, k))
            except AssertionError as e:
                raise AssertionError(f"{name} {method} k_out={k}") from e


def fuse_on_device(idx, lists, k, want_count=True, **kw):
    """Mi355Index.fuse_lists_device over buffers of this call"""
    v1, i1, v2, i2 = (np.ascontiguousarray(a, dtype=t) for a, t in zip(lists, (np.float64, np.int64) * 2))
    maps = [None if kw.get(m) is None else np.ascontiguousarray(kw[m], dtype=np.int64) for m in ("map1", "map2")]
    B = v1.shape[0]
    out = np.empty((B, k)), np.empty((B, k), dtype=np.int64), np.empty(B, dtype=np.int32)
    host = [v1, i1, v2, i2, *maps, *out]
    bufs = [None if a is None else idx.dev_alloc(max(a.nbytes, 8)) for a in host]
    try:
        for p, a in zip(bufs[:6], host[:6]):
            if a is not None and a.nbytes:
                idx.dev_upload(p, a)
        idx.fuse_lists_device(bufs[0], bufs[1], v1.shape[1], bufs[2], bufs[3], v2.shape[1], B, k, bufs[6], bufs[7],
                              bufs[8] if want_count else None, map1_ptr=bufs[4], map1_len=0 if maps[0] is None else len(maps[0]),
                              map2_ptr=bufs[5], map2_len=0 if maps[1] is None else len(maps[1]),
                              **{n: v for n, v in kw.items() if n not in ("map1", "map2")})
        for p, a in zip(bufs[6:] if want_count else bufs[6:8], out):
            idx.dev_download(p, a)
    finally:
        for p in bufs:
            if p is not None:
                idx.dev_free(p)
    return out if want_count else (out[0], out[1], None)


@pytest.mark.parametrize("method", fuse_ref.METHODS)
def test_device_form_equals_the_reference(idx, method):
    for i, (name, lists, kw) in enumerate(INPUTS):
        want, k = want_of(i, method), k_top(lists)
        try:
            same(fuse_on_device(idx, lists, k, **keywords(lists, kw, method)), want)
        except AssertionError as e:
            raise AssertionError(f"{name} {method}") from e
    _, lists, kw = INPUTS[1]
    got = fuse_on_device(idx, lists, 2, want_count=False, **keywords(lists, kw, method))   # no counter: none is written
    assert np.array_equal(got[1], want_of(1, method)[1][:, :2])


def test_an_exact_rrf_tie_goes_to_the_document_seen_first(idx):
    # rank 2 of list 1 (id 7) and rank 2 of list 2 (id 9) are in one list each: the same f; so are the two rank-3 documents
    v1, i1 = [[0.1, 0.2, 0.3]], [[5, 7, 8]]
    v2, i2 = [[-3.0, -2.0, -1.0]], [[5, 9, 6]]
    kw = dict(method="rrf", modes=("one_minus", "negate"), rrf_k=60, fetch_k=3)
    got = idx.fuse_lists(v1, i1, v2, i2, 6, **kw)
    assert got[1].tolist() == [[5, 7, 9, 8, 6, -1]] and got[2].tolist() == [5]
    assert got[0][0, 1] == got[0][0, 2] and got[0][0, 3] == got[0][0, 4]
    same(got, fuse_ref.fuse_lists(v1, i1, v2, i2, 6, **kw))
    got = idx.fuse_lists(v2, i2, v1, i1, 6, **{**kw, "modes": ("negate", "one_minus")})   # the other list first: 9 before 7
    assert got[1].tolist() == [[5, 9, 7, 6, 8, -1]]
    # a convex-combination tie: with weight 0 the first list's documents all score the floor
    got = idx.fuse_lists(v1, i1, [[-1.0]], [[4]], 4, method="mm", modes=("one_minus", "negate"), weight=0.0)
    assert got[1].tolist() == [[4, 5, 7, 8]]


def _stats(idx):
    return idx.stat("fuse_calls"), idx.stat("fuse_queries")


def test_stats_count_calls_and_queries(idx):
    idx.reset_stats()
    assert _stats(idx) == (0, 0)
    _, lists, kw = INPUTS[1]
    idx.fuse_lists(*lists, 3, **keywords(lists, kw, "rrf"))
    assert _stats(idx) == (1, 3)
    fuse_on_device(idx, lists, 3, **keywords(lists, kw, "mm"))
    assert _stats(idx) == (2, 6)
    empty = np.empty((0, 4)), np.empty((0, 4), dtype=np.int64)
    v, i, c = idx.fuse_lists(*empty, *empty, 2, method="rrf")      # B == 0: a valid no-op
    assert v.shape == (0, 2) and i.shape == (0, 2) and c.shape == (0,) and _stats(idx) == (2, 6)


def test_refusals_change_nothing(idx):
    from autorag_research_amd._native import FuseOpts

    lib, h = idx._lib, idx._h
    B, w = 2, 1025
    v = np.tile(np.linspace(0.0, 1.0, w), (B, 1))
    i = np.tile(np.arange(w, dtype=np.int64), (B, 1))
    out_v, out_i, out_c = np.empty((B, 2049)), np.empty((B, 2049), dtype=np.int64), np.empty(B, dtype=np.int32)
    f64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    i64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))  # noqa: E731
    i32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))  # noqa: E731
    nan, inf = float("nan"), float("inf")

    def raw(opts=(0, 0, 1, 60, 4, 0.5, 0.0, 0.0), **kw):
        a = dict(v1=f64(v), i1=i64(i), w1=4, m1=None, n1=0, v2=f64(v), i2=i64(i), w2=3, m2=None, n2=0, B=B, k=5,
                 o=None if opts is None else ctypes.byref(FuseOpts(*opts)), ov=f64(out_v), oi=i64(out_i), oc=i32(out_c))
        a.update(kw)
        return lib.mi355dr_fuse_lists(h, a["v1"], a["i1"], a["w1"], a["m1"], a["n1"], a["v2"], a["i2"], a["w2"], a["m2"], a["n2"],
                                      a["B"], a["k"], a["o"], a["ov"], a["oi"], a["oc"])

    idx.reset_stats()
    assert raw() == 0 and _stats(idx) == (1, 2)                   # (the call the refusals vary is a valid one)
    invalid = [dict(B=-1), dict(w1=0), dict(w2=-3), dict(k=0), dict(v1=None), dict(i2=None), dict(ov=None), dict(oi=None),
               dict(opts=None), dict(m1=i64(i), n1=-1),
               dict(opts=(5, 0, 1, 60, 4, 0.5, 0.0, 0.0)), dict(opts=(-1, 0, 1, 60, 4, 0.5, 0.0, 0.0)),      # method
               dict(opts=(0, 3, 1, 60, 4, 0.5, 0.0, 0.0)), dict(opts=(0, 0, -1, 60, 4, 0.5, 0.0, 0.0)),      # mode
               dict(opts=(0, 0, 1, -1, 4, 0.5, 0.0, 0.0)), dict(opts=(0, 0, 1, 5, -6, 0.5, 0.0, 0.0)),       # rrf_k, the far rank
               dict(opts=(1, 0, 1, 60, 4, nan, 0.0, 0.0)), dict(opts=(3, 0, 1, 60, 4, inf, 0.0, 0.0)),       # weight
               dict(opts=(2, 0, 1, 60, 4, 0.5, nan, 0.0)), dict(opts=(2, 0, 1, 60, 4, 0.5, 0.0, -inf))]      # tmm minima
    for kw in invalid:
        assert raw(**kw) == E_INVALID, kw
    for kw in (dict(w1=1025), dict(w2=1025), dict(k=2049)):
        assert raw(**kw) == E_UNSUPPORTED, kw
    assert raw(opts=(0, 0, 1, 60, 4, nan, nan, nan)) == 0         # (RRF reads neither the weight nor the minima)
    assert raw(B=0, v1=None, i1=None, v2=None, i2=None, ov=None, oi=None) == 0
    assert lib.mi355dr_fuse_lists_device(h, None, None, 4, None, 0, None, None, 3, None, 0, 2, 5, ctypes.byref(FuseOpts(0, 0, 1, 60, 4, 0.5, 0, 0)),
                                         None, None, None, None) == E_INVALID
    assert _stats(idx) == (2, 4)                                  # the two valid calls, none of the refused ones
    _, lists, kw = INPUTS[5]
    same(idx.fuse_lists(*lists, 7, **keywords(lists, kw, "dbsf")), cut(want_of(5, "dbsf"), 7))
    with pytest.raises(ValueError):
        idx.fuse_lists(*lists, 7, method="softmax")
    with pytest.raises(ValueError):
        idx.fuse_lists(*lists, 7, method="tmm", mins=(0.0, None))
