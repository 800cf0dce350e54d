"""GPU: `bench.py --full` keeps the driver's contract -- ONE JSON line, last on stdout, with the keys the driver reads, the
`roofline` and `cpu_baseline` objects, and the bench's own parity verdicts true -- on a corpus small enough to run inside the
suite (the driver runs the full-size line itself).  A second run takes the distributed code path with a world of one
(process group on RCCL, packed all-gather + merge inside the timed loop, the sharded answer compared with one GPU's).  A plain
run (no `--full`) prints the headline line alone, and `--dump-outputs` writes the last timed step's answer."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TOP_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline"}


def _bench(*args, env=None):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], cwd=ROOT, env=e, capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    return json.loads(lines[-1])  # the JSON line is the LAST line of stdout


def test_default_shape_line_on_a_small_corpus(native_built):
    d = _bench("--full", "--rows", "500000", "--steps", "4", "--warmup", "1", "--cpu-sample-rows", "250000", "--cpu-sample-queries",
               "1024")
    assert TOP_KEYS <= set(d), TOP_KEYS - set(d)
    assert d["metric"] == "queries/sec" and d["unit"] == "queries/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 1 and d["vs_baseline"] is None
    assert d["data"] == "synthetic" and d["dtype"] == "f32" and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - d["config"]["queries_per_step"] / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and r["peak"] > 0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and "traffic" in r and r["launches"] > 0
    if r["traffic_source"].startswith("MEASURED"):            # (rocprofv3 present: the PMC sub-run of this same workload)
        rows_per_launch = d["config"]["rows_total"] / (r["launches"] / d["steps"])
        assert 0.9 * 768 * rows_per_launch < r["traffic"] < 1.3 * 768 * rows_per_launch   # the int8 shadow, read about once
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["value"] > 0 and c["cores"] >= 1 and c["sample"]
    assert c["parity_on_sample"] is True                      # the GPU lists equal the oracle's on the sample, bit for bit
    x = d["extra"]
    assert x["fallback_queries"] == 0 and x["pcie_inclusive"]["queries_per_s"] < d["value"] * 1.05
    # the PCIe-inclusive rate is a top-level sibling of `value`; the >= 2 s sustained figure sits next to the burst
    v = d["value_pcie_inclusive"]
    assert v["unit"] == "queries/s" and 0 < v["value"] < d["value"] * 1.05 and v["ms_per_step"] > 0
    # the power-cap argument is observable in the line itself: the bare stream of the screen's MFMA instruction, measured in this
    # run on this chip, and the screen's fraction of it DERIVED from that measurement (not from a constant of another box)
    bs = r["bare_stream"]
    assert "error" not in bs, bs
    assert bs["instruction"] == "v_mfma_i32_32x32x32_i8" and 1500 < bs["tops"] < 5100 and bs["seconds"] >= 2
    assert abs(r["frac_of_power_limited_stream"] - r["achieved"] / bs["tops"]) < 1e-3
    assert r["power_limited_stream"]["rate"] == bs["tops"]
    assert r["kernel"].startswith("k_screen_rq<int8>")        # d = 768 int8: the register-resident-query form
    if "error" not in x["power_probe"]:
        assert d["sustained"] == x["sustained"]               # top-level: the driver's parsed record keeps it
        su = x["sustained"]
        assert su["seconds"] >= 1.5 and su["steps"] >= 20 and su["ms_per_step"] > 0
        assert abs(su["queries_per_s"] - su["steps"] * d["config"]["queries_per_step"] / su["seconds"]) <= 1e-3 * su["queries_per_s"]
    assert x["other_k"]["k"] == 100 and x["other_k"]["fallback_queries"] == 0 and x["other_k"]["queries_per_s"] > 0
    assert "power_probe" in x and ("socket_power_W_median" in x["power_probe"] or "error" in x["power_probe"])
    assert d["ndcg_at_10"]["sample_check"]["identical"] is True   # planted answers: GPU ids / nDCG == the oracle's on the sample


def test_distributed_code_path_with_a_world_of_one(native_built):
    d = _bench("--full", "--rows", "500000", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--force-dist",
               env={"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29541", "RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1"})
    assert d["n_gpus"] == 1 and d["config"]["layout"]["row_shards"] == 1
    assert d["extra"]["identical_to_one_gpu"] is True         # all-gather + merge of one shard == the plain search
    # the searches run on an explicit non-default stream (a null handle would make the library use its own stream, which the
    # `wait_event(gather_done)` that protects the double-buffered packed blocks does not order), and the line says how many
    # ranks the collective spans
    c = d["config"]["collective"]
    assert c["search_stream_handle_nonzero"] is True and c["ranks_in_all_gather"] == 1


def test_distributed_code_path_through_the_library_communicator(native_built):
    d = _bench("--full", "--rows", "500000", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--force-dist", "--comm", "lib",
               env={"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29542", "RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1"})
    c = d["config"]["collective"]
    assert c["rccl_comm_count"] == 1 and c["ranks_in_all_gather"] == 1   # ncclCommCount, asked of RCCL itself
    assert d["extra"]["identical_to_one_gpu"] is True


def test_maxsim_leg_reports_the_mfma_roofline_from_the_timed_steps(native_built):
    """`--workload maxsim`: bound "mfma", algorithmic <= issued flops, both below the dense bf16 peak -- the counters are those of
    the TIMED steps (round 4: they were read behind the power probe's extra steps once and the issued rate came out at 4 PF)."""
    d = _bench("--full", "--workload", "maxsim", "--tokens", "text", "--docs", "60000", "--steps", "6", "--warmup", "1",
               "--no-cpu-baseline")
    assert d["metric"] == "queries/sec" and d["value"] > 0 and "workload" in d["config"]
    r = d["roofline"]
    # (round 6: a store of passages is screened over its granule-packed copy -- the line names the kernel and the copy it multiplied)
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["kernel"] == "k_maxsim16_wg8" and "granule-packed" in r["token_copy"]
    assert r["launches"] == 6 and 0 < r["achieved"] <= r["issued_tflops"] * 1.001 < r["peak"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and 0 < r["frac_of_power_limited_stream"] < 1.3
    assert d["extra"]["exact_full_scan_fallbacks"] == 0 and 0 < d["extra"]["candidates_per_query"] < 2000
    # the padded copy on request: the same algorithmic flops over more issued ones, the same answers' statistics
    d0 = _bench("--workload", "maxsim", "--tokens", "text", "--docs", "60000", "--steps", "6", "--warmup", "1", "--no-cpu-baseline",
                "--no-extras", "--opt", "maxsim_pack8=0")
    r0 = d0["roofline"]
    assert r0["kernel"].startswith("k_maxsim16_wg<16>") and r0["token_copy"].startswith("padded")
    assert r0["launches"] == 6 and r0["issued_tflops"] / r0["achieved"] > r["issued_tflops"] / r["achieved"] * 1.05
    assert d0["extra"]["candidates_per_query"] == d["extra"]["candidates_per_query"]


def test_plain_line_and_dumped_outputs(native_built, tmp_path):
    """Without `--full` the line is the headline alone (no CPU baseline, no untimed extras); `--steps` sets the timed steps;
    `--dump-outputs` writes the last timed step's [B,k] distances and row ids, identical from run to run (seeded inputs)."""
    runs = [_bench("--rows", "500000", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / name)) for name in "ab"]
    for d in runs:
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"} <= set(d)
        assert d["metric"] == "queries/sec" and d["unit"] == "queries/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["steps"] == 3 and d["warmup"] == 1 and d["roofline"]["launches"] > 0 and d["extra"]["fallback_queries"] == 0
        assert abs(d["value"] - d["config"]["queries_per_step"] / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
        assert not {"cpu_baseline", "cpu_baselines", "ndcg_at_10", "value_pcie_inclusive", "maxsim", "sustained"} & set(d)
        assert "bare_stream" not in d["roofline"] and d["roofline"]["traffic"] is None
    import numpy as np

    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("distances", "rows")}
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in ("distances", "rows")}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["distances.npy", "rows.npy"]
    assert a["distances"].dtype == np.float64 and a["rows"].dtype == np.float64 and a["rows"].shape == a["distances"].shape == (1024, 10)
    assert (np.diff(a["distances"], axis=1) >= 0).all() and (a["rows"] == np.round(a["rows"])).all()
    assert a["rows"].min() >= 0 and a["rows"].max() < 500_000 and len(np.unique(a["rows"][0])) == 10
    assert all(np.array_equal(a[n], b[n]) for n in a)
