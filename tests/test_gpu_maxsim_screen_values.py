"""GPU: the MaxSim bf16 screen PER DOCUMENT -- every value of every screen form, the bound where it bites, the candidate lists.

Mi355Index.debug_maxsim_pass runs ONE production pass (plan, upload, screen launch, fast path) over screen distances poisoned with
0xFFFFFFFF and hands back what the pass computed and which kernel the launch took.  The reference is maxsim_screen_ref.py (float64
NumPy; imports nothing of the package); the value tolerance is derived there, not tuned.  The searches' own tests compare the final
top-k only: a screen value that is too good over-admits and is hidden by the exact re-score, one that is too bad shows only when
its document belongs in the top-k.

Measured on an MI355X, largest |T - T_ref| / tol per form: one-wave 0.0013, packed 0.0013, workgroup 0.0011, workgroup-packed
0.0007, list 0.0013, generic / list generic 0.0011 (d = 96), 0.0049 (d = 20), 0.0001 (d = 640), persistent rounds 0.0012; the
library's E is 1.000001 x the reference's.  Two scratch mutants fail these tests: the packed one-wave form without its boundary
masking (the value check, at NCB = 1), e_pair without norm_sum * tok_res_max (the bound: |T - S| / E_lib = 1.40).
"""

import functools

import numpy as np
import pytest

import maxsim_screen_ref as ref

pytestmark = pytest.mark.gpu

D = 128
DEFAULTS = {"maxsim_screen": 1, "maxsim_wg": -1, "maxsim_pack8": -1, "maxsim_wg_bps": 4, "maxsim_wg_pipe": 1, "maxsim_wg_min": 8,
            "maxsim_persistent": 0, "maxsim_tighten": 1, "maxsim_subset_screen": -1, "maxsim_aligned": 1, "maxsim_pass_groups": 4}
MS_STATS = ["maxsim_screened", "maxsim_candidates", "maxsim_fallbacks", "maxsim_screen_cols", "maxsim_packed_launches",
            "maxsim_screen_launches", "maxsim_exact_launches", "maxsim_subset_searches", "maxsim_subset_docs",
            "maxsim_subset_screened", "maxsim_subset_exact", "maxsim_subset_fallbacks"]


@pytest.fixture(scope="module")
def pkg(native_built):
    import autorag_research_amd as p

    return p


def _opts(idx, **kw):
    for key, v in {**DEFAULTS, **kw}.items():
        idx.set_option(key, v)


def _unit(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ---- (a) the value stores ------------------------------------------------------------------------------------------------------

LENS_A = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65]


def _boundary_store(seed, n_docs, d, n_long):
    """lengths around every block and granule edge, a few of 300 (10 blocks: across the workgroup forms' stages of 2 and 4 blocks);
    first and last token of every document scaled x 3, so that boundary tokens decide the maxima"""
    rng = np.random.default_rng(seed)
    lens = rng.choice(LENS_A, size=n_docs)
    lens[rng.choice(n_docs, size=n_long, replace=False)] = 300
    off = _offsets(lens)
    tok = _unit(rng, int(off[-1]), d)
    has = lens > 0
    tok[off[:-1][has]] *= 3.0
    tok[off[1:][has] - 1] *= 3.0   # (a single token is scaled twice: still a boundary token)
    return tok, off


class Store:
    """a store, a pool of query vectors, and the per-vector maxima M[i, doc] every query drawn from the pool is summed from"""

    def __init__(self, tok, off, d, pool_seed, pool=512):
        self.tok, self.off, self.d = tok, off, d
        self.lens = np.diff(off)
        self.qpool = _unit(np.random.default_rng(pool_seed), pool, d)
        q16, t16 = ref.bf16_rn(self.qpool), ref.bf16_rn(tok)
        self.M = ref.col_max(q16, t16, off)
        self._q16, self._t16 = q16, t16

    def variant(self, name, n_vec):
        return ref.col_max(self._q16[:n_vec], self._t16, self.off, name)

    def queries(self, qlens):
        """the first sum(qlens) pool vectors as queries of these lengths -> (qtok, qoff, T_ref [B, n_docs], tol [B, n_docs])"""
        qoff = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
        qtok = self.qpool[:qoff[-1]]
        return qtok, qoff, ref.sum_queries(self.M[:qoff[-1]], qoff), ref.tol_ref(qtok, qoff, self.tok, self.off, self.d)

    def add_to(self, idx, split=None):
        """in two add_multivec calls"""
        n = len(self.lens)
        s = n // 2 + 1 if split is None else split
        idx.add_multivec(self.tok[:self.off[s]], self.off[:s + 1])
        idx.add_multivec(self.tok[self.off[s]:], self.off[s:] - self.off[s])


@functools.lru_cache(maxsize=None)
def store_a():
    return Store(*_boundary_store(20260, 700, D, 6), D, pool_seed=1)


@functools.lru_cache(maxsize=None)
def store_generic(d):
    return Store(*_boundary_store(300 + d, 200, d, 2), d, pool_seed=d, pool=128)


@functools.lru_cache(maxsize=None)
def store_rounds():
    rng = np.random.default_rng(83)
    lens = rng.integers(1, 13, size=8300)
    off = _offsets(lens)
    return Store(_unit(rng, int(off[-1]), D), off, D, pool_seed=2, pool=352)


@pytest.fixture(scope="module")
def idx_a(pkg):
    with pkg.Mi355Index(D) as idx:
        store_a().add_to(idx)
        yield idx


def aligned(ncb):
    return [32] * ncb


def unaligned(ncb):
    """query lengths such as [20, 7, 32, ...] that pack into exactly ncb column blocks (3 columns short of full): evenly filled groups of up to
    four queries and 128 columns, as the pass planner packs them"""
    total, out = 32 * ncb - 3, []
    ng = -(-total // 128)
    for i in range(ng):
        g = total // ng + (1 if i < total % ng else 0)
        out += [20, 7, 32, g - 59] if g > 59 else [20, 7, g - 27] if g > 27 else [g]
    assert len(out) <= 16 and sum(out) == 32 * ncb - 3 and min(out) > 0
    return out


RATIOS = {}


def check_values(st, out, qlens, want_form, listed=None, label=None):
    """the four assertions of a value case.  listed: the documents a list form must have written (else: dense)"""
    qtok, qoff, T, tol = st.queries(qlens)
    form = out["form"]
    for key, v in want_form.items():
        assert form[key] == v, (key, form, want_form)
    live = [b for b in range(len(qlens)) if qlens[b] > 0]
    assert [int(x) for x in out["live"]] == [live.index(b) if b in live else -1 for b in range(len(qlens))]
    got = out["screen"]
    assert got.shape == (len(live), len(st.lens))
    bits = got.view(np.uint32)
    has = st.lens > 0
    written = has if listed is None else np.isin(np.arange(len(has)), listed) & has
    worst = 0.0
    for r, b in enumerate(live):
        assert not np.any(bits[r][written] == ref.POISON), "a document the launch should have written holds the poison"
        err = np.abs(got[r][written].astype(np.float64) - T[b][written])
        ratio = err / tol[b][written]
        worst = max(worst, float(ratio.max()))
        bad = np.nonzero(~(ratio <= 1.0))[0]
        assert bad.size == 0, (label, form, "query", b, "docs", np.nonzero(written)[0][bad][:8], "err/tol", ratio[bad][:8])
        if listed is None:
            assert np.all(bits[r][~has] == ref.NAN_BITS), "a document without vectors must hold the kernels' canonical NaN"
        else:
            assert np.all(bits[r][~written] == ref.POISON), "a list form wrote a document that is not listed"
    key = label or form["family"]
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    print(f"[maxsim-screen] {key} ncb={form['ncb']} qlens={list(qlens)[:4]}.. max|T-T_ref|/tol = {worst:.4f}")


def test_reference_is_sensitive_to_boundary_tokens():
    """Reference alone: on the value store, for a query of 64 vectors, >= 99 % of the documents with >= 2 tokens move T_ref by more
    than 100 tol under EACH of: first token dropped, last token dropped, the preceding document's last token added, the following
    document's first token added.  Without this a passing value check would say nothing about boundary blocks.
    (Measured on the CPU: 0.998 / 1.000 / 0.995 / 0.997.  A single 32-vector query reaches 0.978 .. 0.988 with any seed: a document
    of 64 tokens needs some of the query's vectors to have their maximum at a boundary token, and tol grows with the query as the
    shift does.  Every value case below checks every document under up to 16 queries, the unaligned ones 64 and 66 vectors long.)"""
    st = store_a()
    nq = 64
    _, _, T, tol = st.queries([nq])
    for name in ("drop_first", "drop_last", "add_prev", "add_next"):
        Tv = ref.sum_queries(st.variant(name, nq), [0, nq])[0]
        ok = (st.lens >= 2) & ~np.isnan(Tv)
        frac = float(np.mean(np.abs(Tv[ok] - T[0][ok]) > 100.0 * tol[0][ok]))
        print(f"[maxsim-screen] sensitivity {name}: {frac:.4f} of {int(ok.sum())} documents")
        assert ok.sum() >= 500 and frac >= 0.99, (name, frac)


@pytest.mark.parametrize("twin", ["aligned", "unaligned"])
def test_values_d128_one_wave(idx_a, twin):
    """k_maxsim16_d128<NCB, NW, false>, NCB = 1..16: four waves up to 8 column blocks, eight beyond"""
    for ncb in range(1, 17):
        qlens = aligned(ncb) if twin == "aligned" else unaligned(ncb)
        _opts(idx_a, maxsim_wg=0, maxsim_pack8=0)
        qtok, qoff, _, _ = store_a().queries(qlens)
        out = idx_a.debug_maxsim_pass(qtok, qoff, 10)
        check_values(store_a(), out, qlens, {"family": "d128", "ncb": ncb, "waves": 4 if ncb <= 8 else 8}, label="d128 one-wave")


@pytest.mark.parametrize("twin", ["aligned", "unaligned"])
def test_values_d128_packed(idx_a, twin):
    """k_maxsim16_d128<NCB, 4, true> over the granule-packed copy, NCB = 1..4: a document's boundary blocks hold its neighbours' granules"""
    for ncb in range(1, 5):
        qlens = aligned(ncb) if twin == "aligned" else unaligned(ncb)
        _opts(idx_a, maxsim_wg=0, maxsim_pack8=1)
        qtok, qoff, _, _ = store_a().queries(qlens)
        out = idx_a.debug_maxsim_pass(qtok, qoff, 10)
        check_values(store_a(), out, qlens, {"family": "d128_packed", "ncb": ncb, "waves": 4}, label="d128 packed")


@pytest.mark.parametrize("twin", ["aligned", "unaligned"])
@pytest.mark.parametrize("pipe", [0, 1])
@pytest.mark.parametrize("bps", [2, 4])
@pytest.mark.parametrize("wg", [1, 2])
def test_values_workgroup(idx_a, wg, bps, pipe, twin):
    """k_maxsim16_wg<NCB, DEFER, BPS, PIPE>: NCB = 9..16 in the six variants, NCB = 8 (maxsim_wg_min = 8) in its two"""
    for ncb in range(8, 17):
        qlens = aligned(ncb) if twin == "aligned" else unaligned(ncb)
        _opts(idx_a, maxsim_wg=wg, maxsim_wg_bps=bps, maxsim_wg_pipe=pipe, maxsim_pack8=0, maxsim_wg_min=8)
        qtok, qoff, _, _ = store_a().queries(qlens)
        out = idx_a.debug_maxsim_pass(qtok, qoff, 10)
        want = {"family": "wg", "ncb": ncb, "waves": 8, "now": 1 if wg == 2 else 0,
                "bps": 4 if ncb == 8 else bps, "pipe": 1 if ncb == 8 else int(bps == 4 and pipe == 1)}
        check_values(store_a(), out, qlens, want, label="workgroup")


@pytest.mark.parametrize("wg", [-1, 1])
def test_values_workgroup_packed(idx_a, wg):
    """k_maxsim16_wg8 over the granule-packed copy: aligned passes of 8..16 column blocks"""
    for ncb in range(8, 17):
        qlens = aligned(ncb)
        if ncb == 16:
            qlens[-1] = 20   # (the last query of an aligned pass may be shorter)
        _opts(idx_a, maxsim_wg=wg, maxsim_pack8=1, maxsim_wg_min=8)
        qtok, qoff, _, _ = store_a().queries(qlens)
        out = idx_a.debug_maxsim_pass(qtok, qoff, 10)
        check_values(store_a(), out, qlens, {"family": "wg_packed", "ncb": ncb, "waves": 8}, label="workgroup-packed")


def _doc_list(rng, st, frac=0.6):
    """a list with gaps, duplicates, ids outside the store and documents without vectors, in no order -> (ids, the documents it names)"""
    n = len(st.lens)
    pick = np.nonzero(rng.random(n) < frac)[0]
    pick = np.union1d(pick, np.nonzero(st.lens == 0)[0][:5])
    ids = np.concatenate([pick, pick[::7], [-1, n, n + 5, -3, 2 ** 40]]).astype(np.int64)
    return rng.permutation(ids), pick


@pytest.mark.parametrize("twin", ["aligned", "unaligned"])
def test_values_list_d128(idx_a, twin):
    """k_maxsim16_d128<NCB, NW, false, true>: the listed documents where they lie, nothing else written"""
    st = store_a()
    ids, named = _doc_list(np.random.default_rng(5), st)
    assert np.any(st.lens[named] == 0)
    for ncb in (1, 4, 8, 9, 16):
        qlens = aligned(ncb) if twin == "aligned" else unaligned(ncb)
        _opts(idx_a, maxsim_subset_screen=1)
        qtok, qoff, _, _ = st.queries(qlens)
        out = idx_a.debug_maxsim_pass(qtok, qoff, 10, doc_ids=ids)
        check_values(st, out, qlens, {"family": "list_d128", "ncb": ncb, "waves": 4 if ncb <= 8 else 8}, listed=named, label="list d128")


@pytest.mark.parametrize("d", [96, 20, 640])
def test_values_generic_and_list_generic(pkg, d):
    """k_maxsim16<false> / <true>: dims that are not 128-shaped -- 96, 20 (padded to 32), 640 (the widest the screen serves: its query
    fragments fill 160 KiB of LDS exactly, and a launch stages 32 query vectors)"""
    st = store_generic(d)
    ids, named = _doc_list(np.random.default_rng(d), st)
    with pkg.Mi355Index(d) as idx:
        st.add_to(idx)
        for qlens in ([32], [20, 7]) if d == 640 else ([32] * 4, [20, 7, 32], [100, 28]):
            qtok, qoff, _, _ = st.queries(qlens)
            _opts(idx)
            out = idx.debug_maxsim_pass(qtok, qoff, 10)
            check_values(st, out, qlens, {"family": "generic", "waves": 4}, label=f"generic d={d}")
            _opts(idx, maxsim_subset_screen=1)
            out = idx.debug_maxsim_pass(qtok, qoff, 10, doc_ids=ids)
            check_values(st, out, qlens, {"family": "list_generic", "waves": 4}, listed=named, label=f"list generic d={d}")


def test_dim_656_is_not_screened(pkg, oracle):
    """one fragment more than 160 KiB of LDS holds: the pass reports family "none" and the search is the exact scan"""
    rng = np.random.default_rng(656)
    lens = rng.integers(0, 40, size=60)
    off = _offsets(lens)
    tok = _unit(rng, int(off[-1]), 656)
    q = _unit(rng, 20, 656)
    with pkg.Mi355Index(656) as idx:
        idx.add_multivec(tok, off)
        out = idx.debug_maxsim_pass(q, [0, 20], 5)
        assert out["form"]["family"] == "none" and out["lists"] is None and list(out["live"]) == [0]
        d, r = idx.search_maxsim(q, [0, 20], 5)
        wd, wr = oracle.maxsim_topk(tok, off, q, np.array([0, 20], np.int32), 5)
        assert np.array_equal(r, wr) and np.array_equal(d, wd)


@pytest.mark.parametrize("ncb", [1, 11])
def test_values_persistent_rounds(pkg, ncb):
    """maxsim_persistent = 1 over 8 300 documents: more workgroups' worth of documents than are resident at once (512 of the
    four-wave kernel, 256 of the eight-wave one), so the grid is cut and every workgroup walks two rounds"""
    st = store_rounds()
    with pkg.Mi355Index(D) as idx:
        st.add_to(idx)
        _opts(idx, maxsim_persistent=1, maxsim_wg=0, maxsim_pack8=0)
        qlens = aligned(ncb)
        qtok, qoff, _, _ = st.queries(qlens)
        out = idx.debug_maxsim_pass(qtok, qoff, 10)
        nw = 4 if ncb <= 8 else 8
        one_round = -(-len(st.lens) // (nw * 4))
        assert one_round > (512 if nw == 4 else 256)
        check_values(st, out, qlens, {"family": "d128", "ncb": ncb, "waves": nw, "grid": -(-one_round // 2)}, label="d128 persistent")


# ---- the hook itself -----------------------------------------------------------------------------------------------------------

def test_hook_moves_no_stat_and_leaves_the_handle_as_fresh(pkg, oracle):
    st = store_a()
    qtok, qoff, _, _ = st.queries([32, 0, 20, 7])
    ids, _ = _doc_list(np.random.default_rng(9), st)
    res = {}
    for hooked in (True, False):
        with pkg.Mi355Index(D) as idx:
            st.add_to(idx)
            idx.set_option("profile", 1)
            idx.reset_stats()
            if hooked:
                idx.debug_maxsim_pass(qtok, qoff, 10)
                idx.debug_maxsim_pass(qtok, qoff, 100)
                idx.debug_maxsim_pass(qtok, qoff, 10, doc_ids=ids)
                assert {s: idx.stat(s) for s in MS_STATS} == {s: 0 for s in MS_STATS}
            a = idx.search_maxsim(qtok, qoff, 10)
            b = idx.search_maxsim_subset(qtok, qoff, 10, ids)
            res[hooked] = (a, b, {s: idx.stat(s) for s in MS_STATS + ["maxsim_packed_blocks", "maxsim_packed_built"]})
    for i in (0, 1):
        for x, y in zip(res[True][i], res[False][i]):
            assert np.array_equal(x, y, equal_nan=True)
    assert res[True][2] == res[False][2]
    assert res[False][2]["maxsim_screen_launches"] == 1   # (option "profile" was still on after the hook)
    wd, wr = oracle.maxsim_topk(st.tok, st.off, qtok, qoff, 10)
    live = np.array([True, False, True, True])
    assert np.array_equal(res[True][0][1][live], wr[live]) and np.array_equal(res[True][0][0][live], wd[live])


def test_hook_refuses_what_is_not_one_pass(pkg):
    st = store_a()
    with pkg.Mi355Index(D) as idx:
        st.add_to(idx)
        want = idx.search_maxsim(st.qpool[:32], [0, 32], 10)
        for qlens in ([8] * 17, [128] * 4 + [8], [129], [32] * 5):
            qoff = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
            k = 100 if qlens == [32] * 5 else 10   # (k > 64: a pass is its first group of four)
            with pytest.raises(pkg.NativeError) as e:
                idx.debug_maxsim_pass(st.qpool[:qoff[-1]], qoff, k)
            assert e.value.code == -1   # MI355DR_E_INVALID
        with idx.view(doc_ids=np.arange(50)) as v, pytest.raises(pkg.NativeError):
            v.debug_maxsim_pass(st.qpool[:32], [0, 32], 10)
        got = idx.search_maxsim(st.qpool[:32], [0, 32], 10)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- (b) the bound, where it bites ---------------------------------------------------------------------------------------------

def _midpoint_vectors(rng, n, f, sign, scale=1.0):
    """components (1 + f 2^-8) 2^e, e in -2..1, one sign pattern: every component sits just under a bf16 rounding midpoint, all
    residuals point the same way and add coherently in every dot product"""
    e = rng.integers(-2, 2, size=(n, D))
    return ((1.0 + f * 2.0 ** -8) * 2.0 ** e * sign[None, :] * scale).astype(np.float32)


def _midpoint_case(f):
    rng = np.random.default_rng(int(f * 100))
    sign = np.where(rng.random(D) < 0.5, -1.0, 1.0)
    lens = np.full(150, 40)
    tok = _midpoint_vectors(rng, int(lens.sum()), f, sign)
    qlens = [32, 24, 9]
    qtok = _midpoint_vectors(rng, sum(qlens), f, sign)
    return rng, sign, tok, _offsets(lens), qtok, np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)


def _bound_ratio(qtok, qoff, tok, off):
    T, S, E = ref.T_ref(qtok, qoff, tok, off), ref.S_ref(qtok, qoff, tok, off), ref.E_ref(qtok, qoff, tok, D)
    return float(np.nanmax(np.abs(T - S) / E[:, None]))


@pytest.mark.parametrize("f", [0.99, 0.5])
def test_bound_holds_where_it_bites(pkg, f):
    """|T - S| <= E_lib, and E_lib = E_ref to 10^-5 both ways (the library can neither understate the bound nor pass by inflating
    it), on data whose bf16 residuals are as large as they get and all add up; again after a second add of 100 x larger tokens,
    after a set_multivec to a document of larger norm and residual, and after removing the document that held the maxima (they
    only grow: the upper comparison is dropped there).
    Non-vacuity, on the reference alone: max |T_ref - S| / E_ref = 0.699 (f = 0.99) and 0.705 (f = 0.5) in NumPy on the development
    machine's CPU (asserted >= 0.5): a bound understated by 2 x fails."""
    rng, sign, tok, off, qtok, qoff = _midpoint_case(f)
    ratio = _bound_ratio(qtok, qoff, tok, off)
    print(f"[maxsim-screen] bound f={f}: max|T_ref - S| / E_ref = {ratio:.4f}")
    assert ratio >= 0.5

    def check(idx, tok, off, upper=True, what=""):
        out = idx.debug_maxsim_pass(qtok, qoff, 10)
        assert out["form"]["family"] != "none"
        S = ref.S_ref(qtok, qoff, tok, off)
        live = np.diff(off) > 0
        E_ref = ref.E_ref(qtok, qoff, tok[np.repeat(live, np.diff(off))] if not live.all() else tok, D)
        E_lib = out["two_e"].astype(np.float64) / 2.0
        gap = np.abs(out["screen"].astype(np.float64) - S)[:, live]
        print(f"[maxsim-screen] bound f={f} {what}: max|T - S| / E_lib = {float((gap / E_lib[:, None]).max()):.4f}, E_lib / E_ref = {E_lib / E_ref}")
        assert np.all(gap <= E_lib[:, None]), what
        assert np.all(E_lib >= E_ref * (1.0 - 1e-5)), (what, E_lib, E_ref)
        if upper:
            assert np.all(E_lib <= E_ref * (1.0 + 1e-5)), (what, E_lib, E_ref)

    with pkg.Mi355Index(D) as idx:
        idx.add_multivec(tok, off)
        check(idx, tok, off, what="built")
        tok2 = _midpoint_vectors(rng, 10 * 40, f, sign, scale=100.0)
        idx.add_multivec(tok2, _offsets([40] * 10))
        tok, off = np.concatenate([tok, tok2]), _offsets([40] * 160)
        check(idx, tok, off, what="after an add of 100 x larger tokens")
        big = _midpoint_vectors(rng, 40, 0.999, sign, scale=1024.0)
        idx.set_multivec([7], big, [0, 40])
        tok = tok.copy()
        tok[7 * 40:8 * 40] = big
        check(idx, tok, off, what="after a set to a larger document")
        idx.remove_multivec([7])
        lens = np.full(160, 40)
        lens[7] = 0
        tok = np.concatenate([tok[:7 * 40], tok[8 * 40:]])
        check(idx, tok, _offsets(lens), upper=False, what="after removing the document that held the maxima")


# ---- (c) the candidate lists, from the returned screen distances themselves ----------------------------------------------------------

def _up(x):
    """x with the kernels' documented upward rounding as slack (the issue's (1 + 10^-6) factor, written for either sign)"""
    return x + abs(x) * 1e-6 + 1e-30


@functools.lru_cache(maxsize=None)
def store_lists(kind):
    rng = np.random.default_rng({"wide": 11, "clustered": 12, "few": 13, "ties": 14}[kind])
    if kind == "wide":       # 2 500 documents: k_ms_select runs two stages
        lens = rng.integers(0, 41, size=2500)
        off = _offsets(lens)
        tok = _unit(rng, int(off[-1]), D)
        q = _unit(rng, 64, D)
    else:
        base = _unit(rng, 20, D)
        docs = []
        if kind == "clustered":  # a few hundred near-duplicates inside the band, exact duplicates for ties at x_k
            for i in range(1500):
                if i % 20 == 0 and len(docs) < 1400:
                    docs.append(base.copy())
                elif i % 4 == 1:
                    noise = rng.standard_normal(base.shape).astype(np.float32)
                    docs.append(base + noise * np.float32(rng.random() * 4e-4))
                elif i % 50 == 7:
                    docs.append(np.zeros((0, D), np.float32))
                else:
                    docs.append(_unit(rng, int(rng.integers(1, 30)), D))
        elif kind == "ties":     # a starter longer than the tightening takes: 1 600 exact duplicates (1 100 of them in a 70 % list)
            docs = [base.copy() if i % 4 != 3 else _unit(rng, 9, D) for i in range(2134)]
        else:                    # fewer documents with vectors than k
            docs = [_unit(rng, 5, D) if i % 5 == 2 else np.zeros((0, D), np.float32) for i in range(25)]
        tok = np.concatenate(docs)
        off = _offsets([len(x) for x in docs])
        q = np.concatenate([base, _unit(rng, 44, D)])
    return tok, off, q


@functools.lru_cache(maxsize=None)
def _exact_all(kind, q0, q1):
    from oracle import cpu_ref

    tok, off, q = store_lists(kind)
    return np.array([cpu_ref.maxsim_distance(tok[off[i]:off[i + 1]], q[q0:q1]) if off[i + 1] > off[i] else np.nan
                     for i in range(len(off) - 1)], dtype=np.float32)


def check_lists(pkg, kind, k, use_list):
    tok, off, q = store_lists(kind)
    lens = np.diff(off)
    n = len(lens)
    qlens = [20, 0, 32]
    qoff = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    qtok = q[:qoff[-1]]
    ids = None
    eligible = lens > 0
    if use_list:
        rng = np.random.default_rng(k)
        pick = np.nonzero(rng.random(n) < 0.7)[0]
        ids = rng.permutation(np.concatenate([pick, pick[::5], [-1, n, n + 9]]).astype(np.int64))
        eligible = eligible & np.isin(np.arange(n), pick)
    with pkg.Mi355Index(D) as idx:
        idx.add_multivec(tok, off)
        for tighten in (0, 1):
            _opts(idx, maxsim_tighten=tighten, maxsim_subset_screen=1)
            out = idx.debug_maxsim_pass(qtok, qoff, k, doc_ids=ids)
            cap, L = out["cand_cap"], out["lists"]
            assert cap == 8192 and out["tighten_max"] == 1024 and L is not None and list(out["live"]) == [0, -1, 1]
            for r, b in enumerate([0, 2]):
                T = out["screen"][r].astype(np.float64)
                two_e = float(out["two_e"][r])
                el = np.nonzero(eligible)[0]
                Ts = np.sort(T[el])
                assert not np.isnan(Ts).any()
                x_k = Ts[k - 1] if len(el) >= k else np.inf
                sets = {}
                for name in ("wide", "starter", "final"):
                    e = L[name][r]
                    sets[name] = set(int(x) for x in e["ids"])
                    assert len(sets[name]) == len(e["ids"]), (name, "entries are not unique")
                    assert e["count"] == len(e["ids"]) and e["overflow"] == int(e["count"] > cap), (name, e["count"], e["overflow"])
                wide_lo = set(int(x) for x in el[T[el] <= x_k + two_e])
                wide_hi = set(int(x) for x in el[T[el] <= _up(x_k + two_e)])
                assert wide_lo <= sets["wide"] <= wide_hi, (kind, k, len(wide_lo), len(sets["wide"]), len(wide_hi))
                exact = _exact_all(kind, int(qoff[b]), int(qoff[b + 1]))
                usable = False
                if tighten:
                    starter = set(int(x) for x in el[T[el] <= x_k]) if len(el) >= k else sets["starter"]
                    assert sets["starter"] == starter, (kind, k, len(starter), len(sets["starter"]))
                    assert np.array_equal(L["wide"][r]["sd"].view(np.uint32), out["screen"][r][L["wide"][r]["ids"]].view(np.uint32))
                    usable = k <= len(starter) <= out["tighten_max"]
                else:
                    assert L["starter"][r]["count"] == 0
                if usable:
                    Dk = float(np.sort(exact[sorted(starter)])[k - 1])
                    w = np.array(sorted(sets["wide"]))
                    fin_lo = set(int(x) for x in w[T[w] <= Dk + two_e / 2.0])
                    fin_hi = set(int(x) for x in w[T[w] <= _up(Dk + two_e / 2.0)])
                    assert fin_lo <= sets["final"] <= fin_hi, (kind, k, len(fin_lo), len(sets["final"]), len(fin_hi))
                else:
                    assert sets["final"] == sets["wide"]
                ex = exact[el]
                top = set(int(x) for x in el[ex <= np.sort(ex)[min(k, len(el)) - 1]])   # the exact top-k, ties included
                assert top <= sets["final"], (kind, k, sorted(top - sets["final"])[:8])
                print(f"[maxsim-screen] lists {kind} k={k} list={use_list} tighten={tighten} q{b}: wide {len(sets['wide'])} "
                      f"starter {len(sets['starter'])} final {len(sets['final'])} exact top {len(top)}")
    return out


@pytest.mark.parametrize("use_list", [False, True])
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("kind", ["wide", "clustered"])
def test_candidate_lists(pkg, kind, k, use_list):
    """wide = every document within 2E of the k-th best screen distance, starter = the screen's top-k with its ties, final = the
    wide list within E of the starter's k-th best exact distance (maxsim_tighten = 0: the wide list); each holds the oracle's
    exact top-k, ties included; entries unique, counts and overflow flags right"""
    check_lists(pkg, kind, k, use_list)


@pytest.mark.parametrize("use_list", [False, True])
def test_candidate_lists_fewer_documents_than_k(pkg, use_list):
    """every document with vectors is a candidate; no usable starter: the final list is the wide list"""
    check_lists(pkg, "few", 10, use_list)


@pytest.mark.parametrize("use_list", [False, True])
def test_candidate_lists_starter_beyond_the_tightening(pkg, use_list):
    """more than a thousand exact duplicates tie at x_k: a starter of more than kMsTightenMax = 1024 entries is not used, final = wide"""
    out = check_lists(pkg, "ties", 10, use_list)
    assert out["lists"]["starter"][0]["count"] > 1024


def test_candidate_lists_overflow(pkg):
    """8 300 identical documents: every list would hold more than kMsCandCap = 8192 entries -- counts run on, the flags are set,
    the lists hold their first 8192"""
    rng = np.random.default_rng(15)
    doc = _unit(rng, 2, D)
    tok = np.tile(doc, (8300, 1))
    off = _offsets([2] * 8300)
    with pkg.Mi355Index(D) as idx:
        idx.add_multivec(tok, off)
        out = idx.debug_maxsim_pass(_unit(rng, 8, D), [0, 8], 10)
        L = out["lists"]
        assert len(np.unique(out["screen"][0].view(np.uint32))) == 1
        for name in ("wide", "starter"):
            e = L[name][0]
            assert e["count"] == 8300 and e["overflow"] == 1 and len(set(e["ids"].tolist())) == 8192, name
        assert L["final"][0]["overflow"] == 1 and L["final"][0]["count"] == 0
