"""GPU: the list forms of the source cap (`mi355dr_collapse_lists`, `mi355dr_collapse_lists_device`; csrc/k_collapse.h) against
the plain walk of tests/collapse_ref.py: values as bits, ids, keys, positions, counts, entries and tails, over the shared inputs
-- every width at which the kernel pads, scans or sorts differently -- and every refusal of the contract."""

import ctypes

import numpy as np
import pytest

import collapse_ref as cr

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


@pytest.fixture(scope="module")
def idx(pkg):
    with pkg.Mi355Index(8) as ix:   # (the list forms read no index state: an empty index serves)
        yield ix


@pytest.fixture(scope="module")
def inputs():
    return [(name, v, i, k, c, cr.collapse(v, i, k, c, i.shape[1])) for name, v, i, k, c in cr.all_inputs()]


def test_host_form_equals_the_walk_on_every_shared_input(idx, inputs):
    for name, vals, ids, keys, cap, exp in inputs:
        cr.same(idx.collapse_lists(vals, ids, keys, cap), exp, "host: " + name)


def test_device_form_equals_the_walk_on_every_shared_input(idx, inputs):
    for name, vals, ids, keys, cap, exp in inputs:
        with idx.upload_keys(np.zeros(0, np.int64) if keys is None else keys) as table:
            cr.same(idx.collapse_lists(vals, ids, table, cap), exp, "device: " + name)


def test_k_out_below_at_and_above_the_kept_count(idx, inputs):
    picked = [t for t in inputs if "mixed keys" in t[0] or "pos%3 cap=2" in t[0] or "one key cap=3" in t[0]]
    assert len(picked) >= 8
    for name, vals, ids, keys, cap, full in picked:
        kept = int(full.count[0])
        for k_out in sorted({1, max(kept, 1), kept + 3, 4096}):
            exp = cr.collapse(vals, ids, keys, cap, k_out)
            cr.same(idx.collapse_lists(vals, ids, keys, cap, k_out), exp, f"host k_out={k_out}: {name}")
            with idx.upload_keys(np.zeros(0, np.int64) if keys is None else keys) as table:
                cr.same(idx.collapse_lists(vals, ids, table, cap, k_out), exp, f"device k_out={k_out}: {name}")


def test_one_list_and_more_lists_than_one_block(idx):
    rng = np.random.default_rng(5)
    w, n_ids = 70, 200
    keys = rng.integers(-1, 12, size=n_ids).astype(np.int64)
    for B in (1, 3, 1030):
        ids = rng.integers(-1, n_ids + 10, size=(B, w)).astype(np.int64)
        ids[3::4, 9:] = -1                                     # every fourth list is short: fewer than k_out are kept
        vals = np.sort(rng.standard_normal((B, w)), axis=1)
        exp = cr.collapse(vals, ids, keys, 2, 10)
        assert B < 1030 or ((exp.count > 10).any() and (exp.count < 10).any())
        cr.same(idx.collapse_lists(vals, ids, keys, 2, 10), exp, f"host B={B}")
        with idx.upload_keys(keys) as table:
            cr.same(idx.collapse_lists(vals, ids, table, 2, 10), exp, f"device B={B}")


def test_each_optional_output_given_and_null(idx):
    rng = np.random.default_rng(6)
    w, n_ids = 130, 150
    keys = rng.integers(-1, 9, size=n_ids).astype(np.int64)
    ids = rng.integers(-1, n_ids, size=(4, w)).astype(np.int64)
    vals = np.sort(rng.standard_normal((4, w)), axis=1)
    exp = cr.collapse(vals, ids, keys, 1, 20)
    flags = ("with_keys", "with_pos", "with_count", "with_entries")
    with idx.upload_keys(keys) as table:
        for off in (*flags, None):
            kw = {f: f != off for f in flags} if off else {f: False for f in flags}
            for form, t in (("host", keys), ("device", table)):
                got = idx.collapse_lists(vals, ids, t, 1, 20, **kw)
                assert [g is None for g in got[2:]] == [not kw[f] for f in flags]
                cr.same(got, exp, f"{form} without {off or 'all four'}")


def test_stats_and_resident_bytes(idx):
    idx.reset_stats()
    vals, ids = np.zeros((2, 5)), np.arange(10, dtype=np.int64).reshape(2, 5)
    idx.collapse_lists(vals, ids, np.zeros(10, np.int64), 1)
    with idx.upload_keys(np.zeros(10, np.int64)) as table:
        idx.collapse_lists(vals, ids, table, 1)
    assert idx.stat("collapse_calls") == 2 and idx.stat("collapse_searches") == 0
    assert idx.stat("hbm_bytes_resident") >= 2 * 5 * 16 + 10 * 8   # (the host form's staging is the index's and is counted)
    idx.collapse_lists(np.zeros((0, 5)), np.zeros((0, 5), np.int64), None, 1)   # B == 0: a no-op that counts nothing
    assert idx.stat("collapse_calls") == 2


def _raw_host(pkg, idx, vals, ids, w, B, keys, keys_len, cap, k_out, outs):
    """mi355dr_collapse_lists with every pointer as given (None = NULL); returns the error code."""
    from autorag_research_amd._native import ptr

    p = lambda a, ct: None if a is None else ptr(a, ct)  # noqa: E731
    return idx._lib.mi355dr_collapse_lists(idx._h, p(vals, ctypes.c_double), p(ids, ctypes.c_int64), w, B, p(keys, ctypes.c_int64),
                                           keys_len, cap, k_out, p(outs[0], ctypes.c_double), p(outs[1], ctypes.c_int64),
                                           p(outs[2], ctypes.c_int64), p(outs[3], ctypes.c_int32), p(outs[4], ctypes.c_int32),
                                           p(outs[5], ctypes.c_int32))


def test_every_refusal_and_a_refused_call_changes_nothing(pkg, idx):
    w, B, k_out = 6, 2, 4
    vals = np.zeros((B, w))
    ids = np.arange(B * w, dtype=np.int64).reshape(B, w)
    keys = np.zeros(B * w, dtype=np.int64)

    def outs():
        return [np.full((B, k_out), 77.0), np.full((B, k_out), 77, np.int64), np.full((B, k_out), 77, np.int64),
                np.full((B, k_out), 77, np.int32), np.full(B, 77, np.int32), np.full(B, 77, np.int32)]

    ok = dict(vals=vals, ids=ids, w=w, B=B, keys=keys, keys_len=len(keys), cap=1, k_out=k_out)
    wide_v, wide_i = np.zeros((1, 4097)), np.zeros((1, 4097), np.int64)
    cases = [
        ("B < 0", dict(B=-1), E_INVALID), ("w <= 0", dict(w=0), E_INVALID), ("cap <= 0", dict(cap=0), E_INVALID),
        ("cap < 0", dict(cap=-3), E_INVALID), ("k_out <= 0", dict(k_out=0), E_INVALID), ("keys_len < 0", dict(keys_len=-1), E_INVALID),
        ("null vals", dict(vals=None), E_INVALID), ("null ids", dict(ids=None), E_INVALID),
        ("a table of length 0", dict(keys_len=0), E_INVALID), ("a null table with a length", dict(keys=None), E_INVALID),
        ("w > 4096", dict(vals=wide_v, ids=wide_i, w=4097, B=1), E_UNSUPPORTED), ("k_out > 4096", dict(k_out=4097), E_UNSUPPORTED),
    ]
    idx.reset_stats()
    resident = idx.stat("hbm_bytes_resident")
    for name, change, code in cases:
        a = dict(ok, **change)
        o = outs()
        rc = _raw_host(pkg, idx, a["vals"], a["ids"], a["w"], a["B"], a["keys"], a["keys_len"], a["cap"], a["k_out"], o)
        assert rc == code, (name, rc)
        assert all((x == 77).all() for x in o), name   # nothing was written
    for missing in (0, 1):   # a null result buffer with work to do
        o = outs()
        o[missing] = None
        assert _raw_host(pkg, idx, vals, ids, w, B, keys, len(keys), 1, k_out, o) == E_INVALID
        assert all((x == 77).all() for x in o if x is not None)
    assert idx.stat("collapse_calls") == 0 and idx.stat("hbm_bytes_resident") == resident
    # the device form refuses the same way, before it touches a pointer
    buf = idx.dev_alloc(1 << 16)   # (room for every shape below, should a check ever let one through)
    try:
        for args, code in (((buf, buf, 4097, 1, 1, 4, buf, buf), E_UNSUPPORTED), ((buf, buf, 4, 1, 1, 4097, buf, buf), E_UNSUPPORTED),
                           ((buf, buf, 4, 1, 0, 4, buf, buf), E_INVALID), ((0, buf, 4, 1, 1, 4, buf, buf), E_INVALID),
                           ((buf, buf, 4, 1, 1, 4, buf, 0), E_INVALID), ((buf, buf, 4, -1, 1, 4, buf, buf), E_INVALID)):
            with pytest.raises(pkg.NativeError) as e:
                idx.collapse_lists_device(*args)
            assert e.value.code == code, args
        with pytest.raises(pkg.NativeError) as e:
            idx.collapse_lists_device(buf, buf, 4, 1, 1, 4, buf, buf, keys_ptr=buf, keys_len=0)
        assert e.value.code == E_INVALID
    finally:
        idx.dev_free(buf)
    assert idx.stat("collapse_calls") == 0
    # B == 0 with null pointers everywhere is a valid no-op; and the good call still works after all of this
    assert _raw_host(pkg, idx, None, None, w, 0, None, 0, 1, k_out, [None] * 6) == 0
    o = outs()
    assert _raw_host(pkg, idx, vals, ids, w, B, keys, len(keys), 1, k_out, o) == 0
    cr.same(tuple(o), cr.collapse(vals, ids, keys, 1, k_out), "after the refusals")


def test_the_list_forms_are_allowed_on_a_view(pkg):
    rng = np.random.default_rng(8)
    C = rng.standard_normal((300, 16)).astype(np.float32)
    with pkg.Mi355Index(16) as parent:
        parent.add(C)
        with parent.view(row_ids=np.arange(0, 300, 3)) as v:
            vals = np.sort(rng.standard_normal((2, 40)), axis=1)
            ids = rng.integers(0, 300, size=(2, 40)).astype(np.int64)
            keys = (np.arange(300) // 10).astype(np.int64)
            cr.same(v.collapse_lists(vals, ids, keys, 1, 12), cr.collapse(vals, ids, keys, 1, 12), "on a view")
