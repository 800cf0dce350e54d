"""CPU: the m(k) table the library compiles in for its speculative pass (csrc/dev_common.h kSpecM) is what the rule of
tools/spec_model.py gives -- the smallest m whose mean miss margin is five of its standard deviations at n = 2^20 and n = 10^7,
d = 768 -- and every enabled k is inside the one-wave prune's budget.  Quadrature only: no simulation, no device."""

import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("spec_model", ROOT / "tools" / "spec_model.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def compiled(native_built):
    from autorag_research_amd import _native

    lib = _native.load()
    return [lib.mi355dr_debug_spec_m(k) for k in range(0, 40)]


def test_compiled_table_is_the_rule(model, compiled):
    want = model.table()
    assert compiled[:len(want)] == want
    assert all(m == 0 for m in compiled[len(want):])  # (no k above the starter's range speculates)
    assert compiled[10] > 0  # the reference's default limit speculates


def test_enabled_k_are_inside_the_budget(model, compiled):
    for k, m in enumerate(compiled):
        if m:
            assert m > k and model.INFLATION * m <= 0.75 * (model.PRUNE_ENTRIES - k), (k, m)
    assert compiled[24] == 0  # (what tests/test_gpu_speculative.py relies on for its ladder case)


def test_rule_at_k10_matches_the_margins_it_is_derived_from(model):
    sc = model.Scores(model.RULE_D)
    m = model.smallest_m(10, sc)
    for n in model.RULE_NS:
        mu, sd, above = model.margin(sc, n, 10, m)
        assert mu >= model.K_SIGMAS * sd and 10 < above < m  # (lighter tails than the Gaussian quantile assumes: fewer than m rows)
    mu, sd, _ = model.margin(sc, model.RULE_NS[1], 10, m - 1)
    assert mu < model.K_SIGMAS * sd  # m is the smallest
