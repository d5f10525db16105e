"""bench.py's launch contract, the parts that need no GPU: `python bench.py --gpus N` without a launcher re-executes itself under
torch.distributed.run (one rank per GPU, 127.0.0.1 rendezvous); every rank pins itself to its own slice of the host's cores; the
roofline helpers agree with SURVEY 8d."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gpus_n_without_a_launcher_reexecutes_under_torch_distributed_run(monkeypatch):
    bench = _bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7
    import subprocess
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False); monkeypatch.delenv("RANK", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7                                      # the launcher's status is the process's status
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_world_size_that_disagrees_with_gpus_is_refused(monkeypatch):
    bench = _bench()
    monkeypatch.setenv("WORLD_SIZE", "2"); monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "WORLD_SIZE=2" in str(e.value.code)


@pytest.mark.skipif(not hasattr(os, "sched_setaffinity"), reason="no affinity API")
def test_every_rank_pins_itself_to_its_own_slice_of_the_cores():
    bench = _bench()
    before = os.sched_getaffinity(0)
    try:
        cores = sorted(before)
        if len(cores) < 2:
            pytest.skip("one core")
        a = bench.pin_rank_to_cores(0, 2)
        os.sched_setaffinity(0, before)
        b = bench.pin_rank_to_cores(1, 2)
        assert a and b and not (set(a) & set(b)) and set(a) | set(b) <= set(cores)
        assert os.sched_getaffinity(0) == set(b)
    finally:
        os.sched_setaffinity(0, before)
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def test_step_floors_follow_the_survey_formula():
    bench = _bench()
    g = bench.train_gflop_per_image(768, 12, 32, 224, 512, 100, 32, True)
    assert abs(g - 17.673449472) < 1e-6
    assert abs(g * 128 / bench.PEAK_TFLOPS_BF16 - 0.9048806) < 1e-5   # ms of MFMA work per bs-128 step (roofline.mfma_floor_ms)
    assert abs(bench.PEAK_TFLOPS_BF16 * 1e12 / (bench.PEAK_HBM_TBS * 1e12) - 312.5) < 1e-9   # the ridge


def test_flush_helper_and_the_dp_schedule_option(monkeypatch, capsys):
    """The JSON line must be the last line of stdout even when a C library has buffered output of its own (the collective library's
    banner): `_flush_c_stdio` empties the process's C stdio buffers and never raises; `--dp-exchange` offers the three schedules and
    defaults to timing the in-stream AND the overlapped one (and the re-exec for `--gpus N` hands the choice on to the ranks)."""
    bench = _bench()
    bench._flush_c_stdio()                                   # callable without a GPU, idempotent
    bench._flush_c_stdio()
    src = open(os.path.join(ROOT, "bench.py")).read()
    # N > 1 default: BOTH the in-stream exchange and the overlapped one are timed, the faster is `value`, both are reported
    assert 'choices=["auto", "single", "staged", "pipelined"], default="auto"' in src
    for field in ("exchange_us_per_step", "per_rank_ms_per_step", "exchange_schedules"):
        assert f'"{field}"' in src
    # the print of the line comes after the process group is gone and the buffers are flushed
    tail = src[src.rindex("destroy_process_group()"):]
    assert "_flush_c_stdio()" in tail and tail.index("_flush_c_stdio()") < tail.index("print(json.dumps(out)")
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"] = cmd
        return 0
    import subprocess
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False); monkeypatch.delenv("RANK", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--dp-exchange", "staged"])
    with pytest.raises(SystemExit):
        bench.main()
    assert "--dp-exchange" in seen["cmd"] and "staged" in seen["cmd"]


def test_dump_outputs_are_float32_npy_within_the_budget_and_sampled_the_same_way_every_run(tmp_path, monkeypatch):
    """`--dump-outputs DIR`: one DIR/<name>.npy per array, float32, DUMP_MAX_BYTES in all; an array over its share of the budget
    becomes a seeded sample of its elements that is the same on every run, so that two builds compare element for element."""
    import numpy as np
    import torch
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    g = torch.Generator().manual_seed(1)
    arrays = {"logits": torch.randn(4, 10, generator=g), "loss": torch.tensor([2.5], dtype=torch.float64),
              "params": torch.randn(5000, generator=g)}
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), arrays)
    assert sorted(os.listdir(tmp_path / "a")) == ["logits.npy", "loss.npy", "params.npy"]
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrays}
    assert all(v.dtype == np.float32 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 4096
    assert np.array_equal(a["logits"], arrays["logits"].numpy()) and float(a["loss"][0]) == 2.5    # small arrays whole
    assert a["params"].size == 4096 // (4 * 3) and np.isin(a["params"], arrays["params"].numpy()).all()
    for n in arrays:
        assert np.array_equal(a[n], np.load(tmp_path / "b" / f"{n}.npy"))


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_what_the_last_step_computed(tmp_path):
    """A plain run is lean: the headline line (ms_per_step = the wall time of one of the K timed steps) and nothing that needs runs
    of its own; --dump-outputs writes the last timed step's results, identical from run to run on the same arguments; --full
    brings the roofline object back."""
    import json
    import subprocess
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--arch", "tiny-256",
            "--batch", "16"]

    def run(*extra):
        out = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout.splitlines()[-1])
    lines = [run("--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for d in lines:
        assert d["steps"] == 4 and d["warmup"] == 2 and d["unit"] == "images/sec" and d["higher_is_better"] is True
        assert abs(d["value"] - 16 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"] and d["dtype"] == "bf16"
        assert not {"roofline", "cpu_baseline", "concurrent_runs", "harness_images_per_sec"} & set(d)
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")}
    assert set(a) == {"logits", "loss", "params", "bn_running_mean", "bn_running_var"}
    assert a["logits"].shape == (16, 100) and a["logits"].dtype == np.float32 and np.isfinite(a["logits"]).all()
    assert abs(float(a["loss"][0]) - lines[0]["config"]["final_loss"]) < 1e-6
    for n, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f"{n}.npy")), n
    full = run("--full", "--no-cpu-baseline")
    assert full["roofline"]["achieved"] > 0 and full["roofline"]["launches_per_step"] > 0


@pytest.mark.gpu
def test_concurrent_runs_side_measurement_is_bit_identical_to_solo_runs():
    """bench.py's `concurrent_runs` object (round 6): K engine contexts on K streams at batch 64 (K = 1, 2, 3) and 128 (K = 1, 2);
    the aggregate rate per K and -- what makes the figure mean anything -- every concurrent run bit-identical to the same run alone."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pevit_amd.synth import ARCHS, synth_state_dict
    bench = _bench()
    arch = ARCHS["tiny-256"]
    out = bench.concurrent_runs_throughput(torch.device("cuda", 0), synth_state_dict(arch, seed=2, text_tower=False), arch, steps=6)
    for bs, ks in (("bs64", ("1", "2", "3")), ("bs128", ("1", "2"))):
        assert out[bs]["bit_identical_to_solo"] is True
        assert tuple(out[bs]["aggregate_images_per_sec_by_runs"]) == ks and all(v > 0 for v in out[bs]["aggregate_images_per_sec_by_runs"].values())
