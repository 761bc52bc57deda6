"""Host-side logic of bench.py (no GPU): argument defaults per workload, the
--dump-outputs writer and the PMC lookups that decide what a line may claim.
One GPU test runs the plain command end to end."""

import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(argv):
    old = sys.argv
    sys.argv = ["bench.py"] + argv
    try:
        return bench.parse()
    finally:
        sys.argv = old


@pytest.mark.parametrize("argv,steps,warmup", [
    ([], 100, 100),                                   # the headline
    (["--steps", "20", "--warmup", "5"], 20, 5),      # the driver's command
    (["--workload", "sdd_dds"], 1000, 1000),          # >= 100 ms of load
    (["--workload", "panel"], 500, 500),
    (["--workload", "moe"], 100, 100),
    (["--workload", "sdd_dds", "--steps", "7"], 7, 1000),
])
def test_step_defaults_per_workload(argv, steps, warmup):
    a = _parse(argv)
    assert (a.steps, a.warmup) == (steps, warmup)


def test_full_and_dump_outputs_are_off_by_default():
    a = _parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.dump_outputs is None
    a = _parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
    for w in ("sweep", "transpose"):  # no floating-point output to write
        with pytest.raises(SystemExit):
            _parse(["--workload", w, "--dump-outputs", "d"])


def test_dump_outputs_float32_fixed_sample_within_budget(tmp_path):
    """A small output is written whole; one over its share of DUMP_BYTES is
    cut to the same sorted sample of whole rows on every call."""
    import numpy as np
    import torch
    gen = torch.Generator().manual_seed(3)
    small = torch.rand(96, 128, generator=gen).to(torch.float16)
    big = torch.rand(8192, 1024, generator=gen).to(torch.bfloat16)
    for d in ("a", "b"):
        bench.dump_outputs({"small": small, "big": big}, str(tmp_path / d), 0, 1)
    s, b = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == b.dtype == np.float32
    assert np.array_equal(s, small.float().numpy())
    share = bench.DUMP_BYTES // 2
    assert b.shape == (share // (1024 * 4), 1024) and b.shape[0] < 8192
    assert s.nbytes + b.nbytes <= bench.DUMP_BYTES <= 64e6
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    # whole rows of the output, in their order: row r of the sample is a row
    # of `big` below every later one
    full = big.float().numpy()
    at = [int(np.flatnonzero((full == row).all(axis=1))[0]) for row in b[:8]]
    assert at == sorted(at) and len(set(at)) == 8
    # at N > 1 every rank writes its own file, on its share of the budget
    bench.dump_outputs({"big": big}, str(tmp_path / "c"), 1, 2)
    r1 = np.load(tmp_path / "c" / "big_rank1.npy")
    assert r1.shape[0] == share // (1024 * 4)


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_its_output(tmp_path):
    """A run without --full times the headline density and nothing else, K
    steps as --steps says, and --dump-outputs writes the C those steps
    computed: the oracle's product of the same seeded operands, rebuilt here
    from the same arguments."""
    import subprocess
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle import oracle as O
    from sputnik_amd import matrix_utils as mu
    from tests import helpers as H
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--m", "640",
            "--k", "512", "--n", "384", "--seed", "5"]
    out = tmp_path / "dump"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv +
                         ["--dump-outputs", str(out)], capture_output=True,
                         text=True, timeout=120, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [x for x in res.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "TFLOP/s"
    assert line["steps"] == 3 and line["warmup"] == 2 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert list(line["by_density"]) == ["0.5"]
    assert line["dense_anchor"] is None and line["cpu_baseline"] is None
    assert line["config1"] is None
    assert [p.name for p in out.iterdir()] == ["c.npy"]
    c = np.load(out / "c.npy")
    assert c.dtype == np.float32 and c.shape == (640, 384)

    a = _parse(argv)
    prob = bench.dsd_panel(a, 1, 0, torch.device("cuda", 0), a.density,
                           m_total=a.m)
    vals = prob.a_vals.float().cpu().numpy().reshape(-1, 128, 128)
    dense = mu.to_dense(640, 512, prob.offsets, prob.indices, vals)
    ref = O.gemm(dense, False, prob.b_vals.float().cpu().numpy().reshape(512, 384),
                 False)
    H.assert_close(c, ref, "f16", "bench --dump-outputs c")


def test_pmc_traffic_needs_same_build_and_shape(tmp_path):
    p = tmp_path / "pmc.json"
    key = "dsd_4096x4096x4096_0.5_f16"
    p.write_text(json.dumps({key: {"build_hash": "abc", "hbm_bytes_per_launch": 123}}))
    assert bench.pmc_traffic(str(p), key, "abc") == (123, "rocprofv3 --pmc, same build")
    b, note = bench.pmc_traffic(str(p), key, "other")
    assert b is None and "other" in note
    # an N > 1 rank's panel (2176 rows) has no entry of its own
    b, note = bench.pmc_traffic(str(p), "dsd_2176x4096x4096_0.5_f16", "abc")
    assert b is None and "no PMC entry" in note
    assert bench.pmc_traffic(str(tmp_path / "missing.json"), key, "abc")[0] is None
