"""CPU: the fusion reference (tests/fuse_ref.py) against the project's host code, and the binding's new surface.

`z` / `dbsf` are restated in fuse_ref by the header's rule (plain left-to-right sums, math.sqrt).  hybrid.cc_fuse takes the
root as `** 0.5` and sums with `sum()`; where `var ** 0.5 == math.sqrt(var)` for both columns and `sum()` is the plain sum
(before Python 3.12), the two must agree bit for bit on every input tests/test_gpu_fuse.py runs.  None of the seeds in
fuse_ref.all_inputs() currently trips the root condition; the test allows at most one query in ten to."""

import math
import struct
import sys

import fuse_ref
from autorag_research_amd import hybrid


def _bits(results):
    return [(r["doc_id"], struct.pack("<d", r["score"])) for r in results]


def test_restated_z_and_dbsf_equal_the_host_code_where_its_arithmetic_is_the_headers():
    total = exempt = 0
    for name, (v1, i1, v2, i2), kw in fuse_ref.all_inputs():
        for q in range(len(v1)):
            r1 = fuse_ref.entries(v1[q], i1[q], kw["modes"][0], kw.get("map1"))
            r2 = fuse_ref.entries(v2[q], i2[q], kw["modes"][1], kw.get("map2"))
            roots_agree = True
            for col in fuse_ref.columns(r1, r2)[1:]:
                live = [s for s in col if s is not None]
                if live:
                    var = fuse_ref.mean_std(live)[2]
                    roots_agree = roots_agree and var ** 0.5 == math.sqrt(var)
            total += 1
            if not roots_agree:
                exempt += 1
                continue
            if sys.version_info >= (3, 12):   # (sum() is compensated there: not the header's sum)
                continue
            for method in ("z", "dbsf"):
                want = hybrid.cc_fuse(r1, r2, kw["weight"], len(r1) + len(r2), method)
                assert _bits(fuse_ref.cc_restated(r1, r2, kw["weight"], method)) == _bits(want), (name, q, method)
    assert total > 1000 and exempt * 10 <= total, (exempt, total)


def test_reference_strikes_ranks_and_orders_by_the_header():
    nan = float("nan")
    # ranks skip the struck-out slots: 11 is rank 1 and 13 rank 2 in list 1; 13 is in both lists, 11 and 20 in one each
    got = fuse_ref.fuse_lists([[nan, 0.5, 0.25, 0.75]], [[10, 11, -1, 13]], [[-3.0, -2.0, -1.0]], [[13, -1, 20]], 5,
                              method="rrf", modes=("one_minus", "negate"), rrf_k=60, fetch_k=4)
    far = 1.0 / 65
    assert got[1].tolist() == [[13, 11, 20, -1, -1]] and got[2].tolist() == [3]
    assert got[0][0, :3].tolist() == [1.0 / 62 + 1.0 / 61, 1.0 / 61 + far, 1.0 / 62 + far]
    # an exact tie (rank 2 in one list each) goes to the document seen first
    got = fuse_ref.fuse_lists([[0.1, 0.2]], [[5, 7]], [[-2.0, -1.0]], [[5, 9]], 3, method="rrf", modes=("one_minus", "negate"),
                              fetch_k=2)
    assert got[1].tolist() == [[5, 7, 9]] and got[0][0, 1] == got[0][0, 2]
    # two empty lists
    got = fuse_ref.fuse_lists([[nan]], [[-1]], [[nan]], [[-1]], 2, method="mm")
    assert got[1].tolist() == [[-1, -1]] and got[2].tolist() == [0]


def test_binding_and_pipelines_carry_the_fusion():
    from autorag_research_amd import _native
    from autorag_research_amd.hybrid import Mi355HybridCCRetrievalPipeline, Mi355HybridRRFRetrievalPipeline
    from autorag_research_amd.index import Mi355Index
    from autorag_research_amd.store import InMemoryStore

    assert {"mi355dr_fuse_lists", "mi355dr_fuse_lists_device"} <= set(_native.ABI_SYMBOLS)
    assert callable(Mi355Index.fuse_lists) and callable(Mi355Index.fuse_lists_device)

    class Child:
        name, retrieval_unit = "child", "chunk"

        async def _retrieve_by_id(self, query_id, top_k):
            return []

    store = InMemoryStore()
    for flag in (None, True, False):
        rrf = Mi355HybridRRFRetrievalPipeline(lambda: store, f"rrf-{flag}", Child(), Child(), device_fusion=flag)
        cc = Mi355HybridCCRetrievalPipeline(lambda: store, f"cc-{flag}", Child(), Child(), normalize_method="tmm",
                                            pipeline_1_min=-1.0, pipeline_2_min=0.0, device_fusion=flag)
        assert rrf.device_fusion is flag and cc.device_fusion is flag
        assert rrf._get_pipeline_config() == {"type": "mi355_hybrid_rrf", "retrieval_unit": "chunk", "retrieval_pipeline_1": "child",
                                              "retrieval_pipeline_2": "child", "rrf_k": 60, "fetch_k_multiplier": 2}
        assert "device_fusion" not in cc._get_pipeline_config()
        assert rrf._retrieve_block(["q"], 2) == [[]]   # (stand-in children: the host path, no GPU touched)
