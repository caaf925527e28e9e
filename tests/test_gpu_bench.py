"""bench.py on the GPU box at small sizes: every configuration prints ONE JSON line with the contract's fields, a roofline
object and, with --full, (cfg2, N = 1) the CPU baseline -- so that a change in the product cannot silently break the line the
driver parses.  A plain run (no --full) measures the timed steps alone; --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
          "dtype", "data", "config", "roofline")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    for f in FIELDS:
        assert f in res, f
    assert res["n_gpus"] == 1 and res["value"] > 0 and res["ms_per_step"] > 0 and res["unit"] == "graphs/sec"
    assert "workload" in res["config"] and res["config"]["library"]["dev_overrides"] == {}
    return res


def test_bench_cfg2_line_small():
    res = _bench("--graphs", "4096", "--steps", "3", "--warmup", "1", "--full")
    rf = res["roofline"]
    assert rf["bound"] == "hbm" and 0 < rf["frac"] < 1 and rf["peak"] == 8000.0
    assert rf["spmm_kernel"]["forward"]["frac"] > 0
    assert "sustained" in rf["box"] and "hbm_probe" in rf["box"]
    cb = res["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1


@pytest.mark.parametrize("cfg,extra", [("cfg4", ["--graphs", "3000", "--batch", "256"]), ("cfg4", ["--graphs", "3000", "--batch", "256", "--padded"]),
                                       ("cfg4", ["--graphs", "3000", "--batch", "256", "--eager"]), ("cfg5", ["--graphs", "2000"]),
                                       ("cfg3", ["--graphs", "32"]), ("cfg1", ["--graphs", "400"]), ("cfg1", ["--graphs", "2000", "--batch", "1024"])])
def test_bench_model_configs_small(cfg, extra):
    res = _bench("--config", cfg, "--steps", "3", "--warmup", "1", "--full", *extra)
    assert cfg in res["config"]["workload"]
    rf = res["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["frac"] is not None and rf["per_call_table"]
    assert rf["unpriced_calls"] == [], rf["unpriced_calls"]


@pytest.mark.parametrize("cfg,extra", [("cfg2", ["--graphs", "4096", "--no-cpu-baseline"]),
                                       ("cfg4", ["--graphs", "3000", "--batch", "256"]), ("cfg5", ["--graphs", "2000"])])
def test_bench_data_parallel_path_with_one_rcc_rank(cfg, extra):
    """The data-parallel path of bench.py as the driver launches it (torch.distributed.run, one process per GPU, RCCL) with the
    ONE rank a 1-GPU box has (--force-dist): process group, flat gradient bucket (= the fused optimiser's gradient buffer for
    cfg4 / cfg5), the all-reduce inside the captured step, the `collective` report with the RCCL version."""
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-dist", "--config", cfg, "--steps", "3",
           "--warmup", "1"] + extra
    for attempt in range(3):                     # a rendezvous on a just-freed port can fail transiently: not what is tested here
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, cwd=ROOT, env=env)
        if r.returncode == 0:
            break
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        cmd[cmd.index("--master-port") + 1] = str(port)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    col = res["collective"]
    assert col["ranks"] == 1 and col["backend"] == "nccl" and col["bucket_floats"] > 0
    assert "rccl_version" in col and col["allreduce_us_standalone"]["median"] > 0
    assert res["value"] > 0 and res["config"]["collective"]


def test_bench_small_batch_reports_a_hipgraph_replay_line():
    """`bench.py --graphs 4096 --graph`: the launch-bound small-batch step also as one hipGraph replay per step (VERDICT r02 item
    5); the contract's `value` stays the eager step, the replay is an extra field."""
    res = _bench("--graphs", "4096", "--graph", "--steps", "20", "--warmup", "3", "--no-cpu-baseline")
    hg = res["hipgraph_replay"]
    assert hg["steps"] == 20 and hg["ms_per_step"] > 0 and hg["value"] > 0
    assert hg["ms_per_step"] <= res["ms_per_step"] * 1.2          # a replay is not slower than the eager launches


def test_bench_plain_run_times_the_steps_alone():
    """Without --full nothing runs after the timed region: no CPU baseline, no SpMM probe, no box probe, no per-call pass."""
    res = _bench("--graphs", "4096", "--steps", "7", "--warmup", "2")
    assert res["steps"] == 7 and res["warmup"] == 2 and res["dtype"] == "f32" and res["higher_is_better"] is True
    rf = res["roofline"]
    assert "cpu_baseline" not in res and rf["spmm_kernel"] is None and "box" not in rf
    assert rf["bound"] == "hbm" and 0 < rf["frac"] < 1           # priced from the timed steps' own events
    res = _bench("--config", "cfg5", "--graphs", "2000", "--steps", "3", "--warmup", "1")
    assert "per_call_table" not in res["roofline"] and "box" not in res["roofline"]


def _dump(tmp_path, tag, *args):
    out = tmp_path / tag
    res = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(out), *args)
    arrays = {f.stem: np.load(f) for f in sorted(out.glob("*.npy"))}
    assert arrays and all(a.dtype == np.float32 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    return res, arrays


def test_bench_dump_outputs_cfg2_is_seeded(tmp_path):
    """--dump-outputs: the layer output, dX (a seeded 2,048-graph sample of the 4,096), dW and dbias of the last timed step;
    the same arguments give the same inputs, so two runs of one build dump the same arrays."""
    _, a = _dump(tmp_path, "a", "--graphs", "4096")
    _, b = _dump(tmp_path, "b", "--graphs", "4096")
    assert set(a) == {"output", "grad_x", "grad_w", "grad_bias"}
    assert a["output"].shape == a["grad_x"].shape == (2048, 32, 64) and a["grad_w"].shape == (64, 64)
    assert a["grad_bias"].size == 64 and np.isfinite(a["grad_x"]).all() and np.abs(a["output"]).max() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    _, c = _dump(tmp_path, "c", "--graphs", "1000")           # a batch at or below the sample size: every graph
    assert c["output"].shape == (1000, 32, 64)


@pytest.mark.parametrize("cfg,extra", [("cfg5", ["--graphs", "2000"]), ("cfg4", ["--graphs", "3000", "--batch", "256", "--eager"])])
def test_bench_dump_outputs_training_step(tmp_path, cfg, extra):
    _, a = _dump(tmp_path, "a", "--config", cfg, *extra)
    assert {"loss", "logits", "param_00"} <= set(a) and np.isfinite(a["loss"]).all()
    assert a["logits"].shape[0] == (2000 if cfg == "cfg5" else 256)
