"""bench.py's launch contract: `--gpus N` either runs N ranks or fails loudly — it never prints an
`n_gpus: 1` line for a request of N > 1.  The CPU half needs no GPU: the refusals happen before any device work."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)


def test_world_size_mismatch_is_refused_before_any_work():
    r = _run(["--gpus", "2"], {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and r.stdout.strip() == "" and "WORLD_SIZE=4 but --gpus 2" in r.stderr


@pytest.mark.skipif(__import__("torch").cuda.device_count() >= 2, reason="needs a box with fewer than 2 GPUs")
def test_more_gpus_than_visible_fails_loudly_without_a_json_line():
    r = _run(["--gpus", "2"])
    assert r.returncode == 3 and r.stdout.strip() == "" and "only" in r.stderr


@pytest.mark.gpu
def test_torchrun_world1_rccl_path_agrees_with_the_plain_run():
    """The launcher path the driver uses for N > 1, at world size 1 with the gradients routed through RCCL (GradSync over a
    one-rank communicator): same step, same line shape, ms_per_step within 25 % of the plain run.  (The N > 1 form is two graphs
    with the flat-buffer all-reduces issued eagerly in between — 8 launches and the host in the loop twice per step: 1.150 against
    1.069 ms on one box (`profiles/r05_bench_rccl_world1_two_graphs.json`), 1.257 against 1.117 ms inside a full-suite run on another;
    the bound checks that the path is the same step, not that it costs nothing.)"""
    common = ["--gpus", "1", "--steps", "40", "--warmup", "10", "--no-cpu-baseline", "--no-extras"]
    plain = _run(common)
    assert plain.returncode == 0, plain.stderr[-2000:]
    a = json.loads(plain.stdout.strip().splitlines()[-1])
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", "29611", BENCH] + common + ["--force-dist"], capture_output=True, text=True, env=env, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    b = json.loads(r.stdout.strip().splitlines()[-1])
    print("plain %.4f ms/step, torchrun + RCCL world-1 %.4f ms/step (%s)" % (a["ms_per_step"], b["ms_per_step"], b["config"]["grad_sync"]))
    assert a["n_gpus"] == b["n_gpus"] == 1 and b["config"]["rccl_nranks"] == 1 and a["config"]["rccl_nranks"] is None
    assert a["dtype"] == b["dtype"] and a["config"]["workload"] == b["config"]["workload"]
    assert abs(b["ms_per_step"] - a["ms_per_step"]) <= 0.25 * a["ms_per_step"], (a["ms_per_step"], b["ms_per_step"])


@pytest.mark.gpu
def test_driver_command_line_shape():
    """The driver's own command with `--full`: ONE JSON line whose headline, `literal_contract`, `protocol`, `roofline` and `cpu_baseline`
    objects are self-consistent (round 6, protocol 3: build -> exactly W untimed + K timed steps = `literal_contract` -> settle replays ->
    W + K again = `value`; every MLP kernel carries its duration inside the step's kernel mix; the CPU baseline states the node's core
    count AND the threads it used)."""
    r = _run(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--no-extras", "--no-pmc", "--cpu-seconds", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["unit"] == "rays/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["data"] == "synthetic" and d["vs_baseline"] is None and "configs[2]" in d["config"]["workload"]
    assert abs(d["value"] - 1024 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    pr, lit = d["protocol"], d["literal_contract"]
    assert pr["version"] == 3 and pr["build_calls_before_warmup"] == 4 and pr["settle_replays_since_build"] == 150 and "sustained" in pr["value_is"]
    assert lit["warmup"] == 5 and lit["steps"] == 20 and abs(lit["value"] - 1024 / (lit["ms_per_step"] * 1e-3)) <= 1e-3 * lit["value"]
    assert 0.8 * d["ms_per_step"] <= lit["ms_per_step"] <= 3.0 * d["ms_per_step"] and 0.05 <= lit["step_frac_mfma"] <= 0.6
    assert "cold_start_ms_per_step" not in d and "setup" not in d
    assert d["launches_per_step"] == 7        # prologue, forward, chain, dW, reduce, fold, Adam
    roof = d["roofline"]
    assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s" and roof["peak"] == 2500.0 and "mlp_bwd_dw_kernel" in roof["kernel"]
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) <= 2e-3 and 0.15 <= roof["frac"] <= 0.45
    assert roof["limited_by"] == "hbm" and 0.4 <= roof["hbm_view"]["frac"] <= 1.0 and "traffic" in roof
    ks = d["roofline_kernels"]
    assert len(ks) == 4 and all(k["in_step_launch_us"] > 0 and k["avg_launch_us"] > 0 for k in ks)
    assert abs(sum(k["in_step_launch_us"] for k in ks) - d["mlp_kernels_us_per_step"]) <= 0.15 * d["mlp_kernels_us_per_step"]
    assert abs(roof["avg_launch_us"] - max(k["in_step_launch_us"] for k in ks)) < 1e-6
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "rays/s" and cb["cores"] >= 1 and cb["value"] > 0 and "oracle" in cb["sample"]
    assert cb["node_cores"] == os.cpu_count() and cb["threads"] == cb["cores"] <= cb["node_cores"] and str(cb["threads"]) in cb["threads_probe_ms"]


@pytest.mark.gpu
def test_plain_run_measures_the_headline_alone():
    """Without `--full` the line carries the headline and what follows from its own steps (`literal_contract`, `protocol`, the step's
    MFMA fraction and launch count); none of the side measurements runs, so the run spends seconds, not minutes, outside its steps."""
    t0 = time.perf_counter()
    r = _run(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["unit"] == "rays/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and "full training step" in d["metric"] and "configs[2]" in d["config"]["workload"]
    assert abs(d["value"] - 1024 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert d["protocol"]["settle_replays_since_build"] == 150 and d["literal_contract"]["steps"] == 20 and d["launches_per_step"] == 7
    side = {"roofline", "roofline_kernels", "roofline_north_star", "mlp_kernels_us_per_step", "traffic_note", "cpu_baseline",
            "render_fwd_rays_per_s_per_gpu", "eval_ms_per_image", "f8_dw_ms_per_step", "fp32_c1_ms_per_step", "ndc_c3_ms_per_step"}
    assert not side & set(d), sorted(side & set(d))
    assert wall - 25 * d["ms_per_step"] * 1e-3 < 60, wall


@pytest.mark.gpu
def test_settle_0_reports_the_literal_contract_as_the_value():
    r = _run(["--gpus", "1", "--steps", "10", "--warmup", "3", "--no-extras", "--no-pmc", "--no-cpu-baseline", "--settle", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["literal_contract"]["ms_per_step"] == d["ms_per_step"] and d["protocol"]["value_is"].startswith("literal_contract")


@pytest.mark.gpu
def test_workload_c3_is_a_main_step_of_its_own():
    """configs[3] per GPU (NDC rays, noise_std 1, black background, 64 + 64) as the main step: what tools/ktrace_step.sh traces."""
    r = _run(["--workload", "c3", "--steps", "10", "--warmup", "3", "--full", "--no-extras", "--no-pmc", "--no-cpu-baseline"])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert "configs[3]" in d["config"]["workload"] and d["config"]["N_importance"] == 64 and d["ms_per_step"] > 0
    assert len(d["roofline_kernels"]) == 4


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path, monkeypatch):
    """--dump-outputs' writer: one DIR/<name>.npy per array, float64 kept, everything else float32; above the byte budget every
    array of more than one row keeps the same seeded sample of rows, identical from call to call."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    arrays = {"a": torch.arange(12, dtype=torch.float32).reshape(4, 3), "b": torch.ones(5, dtype=torch.float64),
              "c": torch.tensor(2.5, dtype=torch.bfloat16), "coarse.sigma.weight": torch.arange(6, dtype=torch.int32)}
    assert bench.dump_outputs(str(tmp_path / "d"), arrays) == sorted(arrays)
    for k, v in arrays.items():
        x = np.load(str(tmp_path / "d" / (k + ".npy")))
        assert x.dtype == (np.float64 if k == "b" else np.float32) and np.array_equal(x, v.float().numpy())
    big = {"x": torch.arange(4000, dtype=torch.float32).reshape(1000, 4), "s": torch.tensor(1.0)}
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    bench.dump_outputs(str(tmp_path / "e"), big)
    bench.dump_outputs(str(tmp_path / "f"), big)
    x, y = np.load(str(tmp_path / "e" / "x.npy")), np.load(str(tmp_path / "f" / "x.npy"))
    assert x.nbytes <= 4000 and x.shape[1] == 4 and np.array_equal(x, y) and np.all(np.diff(x[:, 0]) > 0)
    assert np.load(str(tmp_path / "e" / "s.npy")) == 1.0


@pytest.mark.gpu
def test_dump_outputs_of_the_last_timed_step(tmp_path):
    """`--dump-outputs DIR`: the loss, the PSNR and both models' parameters after the last timed step; the same arguments give the
    same inputs, hence the same outputs, from run to run."""
    import numpy as np
    common = ["--gpus", "1", "--steps", "7", "--warmup", "2", "--settle", "0", "--no-extras", "--no-pmc", "--no-cpu-baseline"]
    outs = []
    for tag in ("a", "b"):
        r = _run(common + ["--dump-outputs", str(tmp_path / tag)])
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert d["steps"] == 7 and d["ms_per_step"] > 0
        names = sorted(f[:-4] for f in os.listdir(str(tmp_path / tag)))
        outs.append({n: np.load(str(tmp_path / tag / (n + ".npy"))) for n in names})
    a, b = outs
    assert sorted(a) == sorted(b) and "loss" in a and "train_psnr" in a and len(a) == 2 + 2 * 24
    assert a["coarse.xyz_encoding_1.0.weight"].shape == (256, 63) and a["fine.rgb.0.bias"].shape == (3,)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for n in a:
        assert np.allclose(a[n], b[n], rtol=1e-5, atol=1e-7), (n, np.abs(a[n] - b[n]).max())
