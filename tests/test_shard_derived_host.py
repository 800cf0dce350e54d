"""CPU: the declaration, export and binding of the sharded range / by-row / MMR entry points, and `ShardedSearcher`'s five
methods over stand-in indexes -- delegation to the local method at world size 1, `NotImplementedError` under `force_pipeline`
for an index without the sharded entry points."""

import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("mi355dr_search_range_sharded_device", "mi355dr_search_rows_sharded_device", "mi355dr_search_range_rows_sharded_device",
         "mi355dr_search_mmr_sharded_device", "mi355dr_mmr_select_sharded")
METHODS = ("search_range", "search_rows", "search_range_rows", "search_mmr", "mmr_select")


def test_header_declares_library_exports_and_native_binds(native_built):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mi355dr.h").read_text(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    from autorag_research_amd import _native

    assert set(NAMES) <= set(_native.ABI_SYMBOLS)
    lib = _native.load()                       # (ctypes resolves a symbol on first use: an unexported one raises here)
    assert lib._name == str(native_built)
    assert [len(getattr(lib, name).argtypes) for name in NAMES] == [9, 8, 10, 9, 9]
    from autorag_research_amd.index import Mi355Index

    for m in ("search_range_sharded_device", "search_rows_sharded_device", "search_range_rows_sharded_device",
              "search_mmr_sharded_device", "search_range_sharded", "search_rows_sharded", "search_range_rows_sharded",
              "search_mmr_sharded", "mmr_select_sharded"):
        assert callable(getattr(Mi355Index, m)), m


def test_header_no_longer_calls_the_sharded_forms_missing():
    text = (ROOT / "include" / "mi355dr.h").read_text()
    assert "Sharding is not built in" not in text
    assert "has to be broadcast first" not in text
    assert text.count("mi355dr_search_range_sharded_device") >= 2 and text.count("mi355dr_search_rows_sharded_device") >= 2


class Recorder:
    """an index stand-in that records the local calls and has none of the sharded entry points"""

    def __init__(self, dim, metric="cosine", device=0):
        self.dim, self.calls = dim, []

    def __len__(self):
        return 0

    def set_option(self, key, value):
        pass

    def close(self):
        pass


def _record(name):
    def method(self, *args):
        self.calls.append((name, args))
        return name

    return method


for _m in METHODS:
    setattr(Recorder, _m, _record(_m))

ARGS = {
    "search_range": (np.zeros((2, 4), dtype=np.float32), [0.5, 0.25], 7),
    "search_rows": (np.array([3, 1]), 5, True),
    "search_range_rows": (np.array([3, 1]), 0.5, 7, True),
    "search_mmr": (np.zeros((2, 4), dtype=np.float32), 3, 9, 0.25),
    "mmr_select": (np.zeros((2, 4), dtype=np.float32), 3, np.array([[1, 2], [3, 4]]), 0.25),
}


@pytest.mark.parametrize("method", METHODS)
def test_world_one_delegates_to_the_local_method_with_the_arguments_unchanged(method):
    from autorag_research_amd.sharded import ShardedSearcher

    s = ShardedSearcher(4, index_factory=Recorder)
    assert s.world == 1
    assert getattr(s, method)(*ARGS[method]) == method
    (name, args), = s.index.calls
    assert name == method and len(args) == len(ARGS[method]) and all(a is b for a, b in zip(args, ARGS[method]))


@pytest.mark.parametrize("method", METHODS)
def test_force_pipeline_without_the_sharded_entry_points_is_not_implemented(method):
    from autorag_research_amd.sharded import ShardedSearcher

    s = ShardedSearcher(4, index_factory=Recorder)
    s.force_pipeline = True
    with pytest.raises(NotImplementedError, match=method):
        getattr(s, method)(*ARGS[method])
    assert s.index.calls == []


def test_defaults_reach_the_local_method():
    from autorag_research_amd.sharded import ShardedSearcher

    s = ShardedSearcher(4, index_factory=Recorder)
    s.search_rows([1], 2)
    s.search_mmr(None, 2, 3)
    assert [a[1:] for _, a in s.index.calls] == [(2, False), (2, 3, 0.5)]
