#!/usr/bin/env python3
"""bench.py -- graphs/sec of the kGCN hot path on synthetic molecular graphs, 1..8 MI355X.

Metric (BASELINE.json): "graphs/sec GraphConv fwd+bwd, 32-node mol graphs x64 feat, 1/2/4/8 GPU".

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfg2|cfg4|cfg5] [--scaling weak|strong]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment LAUNCHES ITS OWN RANKS: it re-executes
itself under torch.distributed.run (one process per GPU, rendezvous on 127.0.0.1, a free port); under a launcher that
already set RANK / WORLD_SIZE it just runs as the rank it is.  Rank 0 prints ONE JSON line either way.

--config cfg2 (default; the configuration BASELINE.json's metric is quoted on): 100,000 random 32-node
    graphs per GPU (random spanning tree + 3 extra edges, symmetrised, + self loops => nnz = 100 exactly), 64-dim
    features, one adjacency channel, kernel [64,64].  One step = kgcn_amd.layers.GraphConv forward, then backward
    producing dX, dW, dbias (+ for N > 1 one RCCL all-reduce of the flat [dW, dbias] bucket).
--config cfg1 (BASELINE config 1, the reference's own CPU-runnable case): example_model/model.py on example_jbl/synthetic.jbl
    (tiled to --graphs (20,000) graphs resident), one step = one mini-batch of --batch (30, example_config/synth.json) graphs:
    device-side assembly, forward, masked softmax CE, backward, all-reduce, TF-Adam as one hipGraph replay.
--config cfg3 (BASELINE config 3): example_model/sparse.py on the kgcn-sparse path: --graphs (128) molecules per GPU as ONE
    block-diagonal adjacency, 128-dim features, widths 256; one step = forward, summed sparse softmax CE, backward,
    all-reduce, TF-Adam on the resident batch.
--config cfg4 (BASELINE config 4): Tox21-shaped multitask training, example_model/model_multitask.py network, N = 50
    padded nodes with true sizes 5..50, F = 81, 12 masked tasks; --graphs molecules resident in HBM per GPU (default
    125,000 = 1 M / 8), one step = one mini-batch of --batch (4,096) molecules per GPU assembled on the device,
    forward, masked sigmoid CE, backward, gradient all-reduce, TF-Adam -- captured in one hipGraph (--eager: plain
    launches).  --padded: compute on all 50 padded rows per molecule like round 2; default: valid rows only.
--config cfg5 (BASELINE config 5): example_model/model_gin.py network at width 256 on 10-node ring graphs
    (data_generator/synth_generator_ring.py distribution), --graphs (20,000) graphs per GPU per step, 256-dim features;
    one step = forward, masked softmax CE, backward, gradient all-reduce, TF-Adam.

Inputs are resident in HBM before the timed region.  --scaling weak (default): every rank owns --graphs graphs /
--batch graphs per step.  --scaling strong (cfg2): --graphs is the GLOBAL batch, sharded contiguously over the ranks
(kgcn_amd.parallel.shard_range); gradients combine with the shard weights.

A plain run sets up, warms up, times --steps steps and prints the line; `ms_per_step` is the wall time of one timed step.
`roofline` prices the dominant kernel against the 8 TB/s HBM peak (cfg2: the fused backward, ALGORITHMIC bytes of
DESIGN.md, median / p10 / p90 of the per-launch HIP-event times inside the timed region).  Everything that needs runs
of its own after the timed region comes with --full only: `roofline.spmm_kernel` (cfg2: the batched SpMM alone -- the
kernel the north-star 60 % target is stated on), `roofline.box` (clocks, power and HBM probe rates under the same
load), the per-call roofline of cfg1 / cfg3 / cfg4 / cfg5 (every C-ABI call of one extra eager step bracketed by HIP
events and priced with its algorithmic bytes / flops, tools/abi_roofline.py; `roofline` is the call with the largest
time) and `cpu_baseline` (cfg2, N = 1): the C restatement of the reference algorithm (oracle/kgcn_ref.c, OpenMP over
graphs) on the host cores on a bounded sample, next to a reference-SHAPED leg (per-graph scipy CSR @ (X W + b) loop,
the op structure of kgcn/layers.py:107-116).

--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step handed its caller as DIR/<name>.npy
(float32; at most 64 MiB in all).  cfg2: `output` and `grad_x` of a fixed, seeded sample of 2,048 graphs (all of them
when the batch is smaller), `grad_w`, `grad_bias`; cfg1 / cfg3 / cfg4 / cfg5: `logits`, `loss` and every parameter
after the update (`param_NN`); --dry: the exchanged gradients (`grad_NN`).  The inputs are seeded: the same arguments
give the same inputs in every run, so that two builds can be compared output for output.

`collective` (N > 1): ranks, backend and RCCL version, bucket size, the all-reduce alone timed with HIP events after the
timed region (and inside the step for cfg2), per-rank step times.

--dry --device cpu --backend gloo: the launcher and the gradient exchange WITHOUT the kernels (dummy gradients of the
configuration's parameter shapes) -- what the CPU test of the multi-rank path runs; the product path itself has no CPU
fallback and `bench.py` without --dry needs a GPU in every rank.
"""
import argparse
import glob
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_NODES = 32
FEAT = 64
EXTRA_EDGES = 3
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
METRIC = "graphs/sec GraphConv fwd+bwd, 32-node mol graphs x64 feat"
DUMP_GRAPHS = 2048             # --dump-outputs, cfg2: graphs of the seeded sample (2 x 16 MiB of output / dX)
DUMP_BUDGET = 64 << 20         # --dump-outputs: bytes in all


# ---------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` spawns its own ranks
# ---------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_command(n, argv, port=None):
    """The command line `python bench.py --gpus n ...` re-executes itself with (one rank per GPU)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
            "--master-addr", "127.0.0.1", "--master-port", str(port or free_port()),
            os.path.abspath(__file__)] + list(argv)


def self_launch(n, argv):
    env = dict(os.environ)
    # HSA_ENABLE_IPC_MODE_LEGACY=0: stated by the build environment of this project ("already exported here and on the GPU box:
    # the host driver only supports dmabuf IPC; without it RCCL / cross-process device-memory sharing fails with
    # hipIpcGetMemHandle: invalid argument") -- never observed by this build on hardware (1-GPU lease), so it is only a DEFAULT:
    # an exported value wins, and the line reports which one the ranks ran with (collective.env).
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # a failing rank must be readable in the launcher's stderr: RCCL warnings on, to stderr (stdout is rank 0's one JSON line)
    env.setdefault("NCCL_DEBUG", "WARN")
    env.setdefault("NCCL_DEBUG_FILE", "/dev/stderr")
    env.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or n) // n)))
    rc = subprocess.call(launch_command(n, argv), env=env)
    if rc != 0:
        print("[bench.py] the %d-rank launch failed with exit code %d: the failing rank's traceback is above, prefixed "
              "'[bench.py rank R/%d]'" % (n, rc, n), file=sys.stderr, flush=True)
    return rc


# ---------------------------------------------------------------------------------------------
# workload generators (build-authored; the reference's synth_generator.py needs edward + TF)
# ---------------------------------------------------------------------------------------------
def gen_mol_graphs(T, n=N_NODES, extra=EXTRA_EDGES, seed=1234):
    """cfg2 (vectorised version of oracle.kgcn_oracle.synth_mol_graphs; same distribution).  Returns flat COO
    (graph, row, col) in row-major order; nnz = T * (2*(n-1+extra) + n)."""
    rng = np.random.default_rng(seed)
    A = np.zeros((T, n, n), np.bool_)
    perm = rng.permuted(np.tile(np.arange(n), (T, 1)), axis=1)
    ar = np.arange(T)
    for i in range(1, n):                                   # random spanning tree
        j = perm[ar, rng.integers(0, i, size=T)]
        A[ar, perm[:, i], j] = True
        A[ar, j, perm[:, i]] = True
    need = np.full(T, extra)
    while (need > 0).any():                                 # extra edges, rejection sampled
        act = np.nonzero(need > 0)[0]
        i = rng.integers(0, n, size=act.size)
        j = rng.integers(0, n, size=act.size)
        ok = (i != j) & ~A[act, i, j]
        a = act[ok]
        A[a, i[ok], j[ok]] = True
        A[a, j[ok], i[ok]] = True
        need[a] -= 1
    A[:, np.arange(n), np.arange(n)] = True                 # self loops
    g, r, c = np.nonzero(A)
    return g.astype(np.int64), r.astype(np.int64), c.astype(np.int64)


def kipf_values(g, r, c, T, n):
    """normalize_adj (kgcn/data_util.py:125-140) on binary symmetric adjacency, float32."""
    deg = np.bincount(g * n + c, minlength=T * n).astype(np.float32)
    deg[deg == 0] = 1
    recip = (1.0 / np.sqrt(deg)).astype(np.float32)
    return (np.float32(1.0) * recip[g * n + r]) * recip[g * n + c]


def gen_tox21_like(G, n=50, seed=4):
    """cfg4: molecules of 5..n atoms on the first `size` node slots of an n-node padded graph: random tree + two extra
    edges + self loops on the real atoms.  Returns (sizes [G], g, r, c flat COO row-major)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(5, n + 1, size=G)
    A = np.zeros((G, n, n), np.bool_)
    ar = np.arange(G)
    for i in range(1, n):
        act = sizes > i
        j = (rng.random(G) * i).astype(np.int64)
        A[ar[act], i, j[act]] = True
        A[ar[act], j[act], i] = True
    for _ in range(2):
        i = (rng.random(G) * sizes).astype(np.int64)
        j = (rng.random(G) * sizes).astype(np.int64)
        A[ar, i, j] = True
        A[ar, j, i] = True
    node = np.arange(n)
    A[:, node, node] = node[None, :] < sizes[:, None]
    g, r, c = np.nonzero(A)
    return sizes, g.astype(np.int64), r.astype(np.int64), c.astype(np.int64), rng


def gen_ring_graphs(G, n=10, seed=5):
    """cfg5, the distribution of data_generator/synth_generator_ring.py:11-46: a 6-ring (even graphs) or 5-ring (odd)
    with self loops on the ring nodes; every (noise node, ring node) pair connected with probability 0.1, symmetric;
    noise nodes carry no self loop.  Returns flat COO (g, r, c) row-major and the labels (ring size 6 -> 0, 5 -> 1)."""
    rng = np.random.default_rng(seed)
    ring = np.where(np.arange(G) % 2 == 0, 6, 5)
    node = np.arange(n)
    in_ring = node[None, :] < ring[:, None]                                       # [G, n]
    A = np.zeros((G, n, n), np.bool_)
    ar = np.arange(G)
    A[:, node, node] = in_ring
    for i in range(6):
        act = ring > i
        j = np.where(i + 1 < ring, i + 1, 0)
        A[ar[act], i, j[act]] = True
        A[ar[act], j[act], i] = True
    noise = (rng.random((G, n, n)) < 0.1) & (~in_ring)[:, :, None] & in_ring[:, None, :]   # (noise row, ring col)
    A |= noise | noise.transpose(0, 2, 1)
    g, r, c = np.nonzero(A)
    return g.astype(np.int64), r.astype(np.int64), c.astype(np.int64), (ring == 5).astype(np.int64), rng


# ---------------------------------------------------------------------------------------------
# algorithmic bytes (SURVEY 8d / DESIGN.md): fp32 values, int32 indices, W/bias on chip
# ---------------------------------------------------------------------------------------------
def algorithmic_bytes(n, din, dout, nnz):
    csr = 4 * (n + 1) + 8 * nnz
    fwd = 4 * n * din + csr + 4 * n * dout
    bwd = 4 * n * dout + csr + 4 * n * din + 4 * n * din     # read g, CSR, read x, write dx
    return dict(csr=csr, fwd=fwd, bwd=bwd, layer=fwd + bwd)


def stats(ms):
    ms = sorted(ms)
    n = len(ms)
    return {"median_ms": ms[n // 2], "p10_ms": ms[n // 10], "p90_ms": ms[(9 * n) // 10], "mean_ms": float(np.mean(ms))}


def dump_outputs(outs, out_dir):
    """--dump-outputs: {name: tensor} -> out_dir/<name>.npy in float32, DUMP_BUDGET bytes at most."""
    arrays = {name: np.asarray(t.detach().cpu().numpy(), dtype=np.float32) for name, t in outs.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BUDGET:
        raise SystemExit("--dump-outputs: %d bytes of outputs, more than the %d allowed" % (total, DUMP_BUDGET))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


# ---------------------------------------------------------------------------------------------
# The state of the box: what the shader clock, the package power and the HBM were during the
# kind of load the timed region puts on the GPU -- so that a reader of the ONE line can tell a slow box from a regression.
# ---------------------------------------------------------------------------------------------
class BoxSensors:
    """Shader clock / memory clock / socket power of one GPU, read from the amdgpu hwmon files (a few microseconds per read)
    or, where they are absent, through amdsmi.  Every failure ends in `source = None` with the reason kept: never raises."""

    def __init__(self, device_index=0):
        self.source, self.why, self._files, self._smi = None, [], {}, None
        try:
            self._find_hwmon(device_index)
        except Exception as e:                                    # noqa: BLE001
            self.why.append("hwmon: %r" % (e,))
        if self.source is None:
            try:
                self._find_amdsmi(device_index)
            except Exception as e:                                # noqa: BLE001
                self.why.append("amdsmi: %r" % (e,))

    def _find_hwmon(self, device_index):
        import glob
        bus = None
        try:
            import torch
            p = torch.cuda.get_device_properties(device_index)
            bus = "%04x:%02x:%02x" % (getattr(p, "pci_domain_id", 0), p.pci_bus_id, p.pci_device_id)
        except Exception:                                         # noqa: BLE001
            pass
        cands = []
        for card in sorted(glob.glob("/sys/class/drm/card[0-9]*")):
            dev = os.path.realpath(os.path.join(card, "device"))
            for hw in glob.glob(os.path.join(dev, "hwmon", "hwmon*")):
                if os.path.exists(os.path.join(hw, "freq1_input")):
                    cands.append((dev, hw))
        if not cands:
            self.why.append("hwmon: no card with freq1_input under /sys/class/drm")
            return
        pick = [c for c in cands if bus and os.path.basename(c[0]).startswith(bus)] or cands[device_index:device_index + 1] or cands[:1]
        dev, hw = pick[0]
        files = {"sclk_mhz": (os.path.join(hw, "freq1_input"), 1e-6), "mclk_mhz": (os.path.join(hw, "freq2_input"), 1e-6)}
        for name in ("power1_average", "power1_input"):
            if os.path.exists(os.path.join(hw, name)):
                files["power_w"] = (os.path.join(hw, name), 1e-6)
                break
        self._files = {k: v for k, v in files.items() if os.path.exists(v[0])}
        float(open(self._files["sclk_mhz"][0]).read())            # must be readable now
        self.source = "hwmon:" + os.path.basename(dev)

    def _find_amdsmi(self, device_index):
        import amdsmi
        amdsmi.amdsmi_init()
        hs = amdsmi.amdsmi_get_processor_handles()
        h = hs[device_index if device_index < len(hs) else 0]
        self._smi = (amdsmi, h)
        if self._read_amdsmi().get("sclk_mhz") is None:
            self._smi = None
            self.why.append("amdsmi: no gfx clock")
            return
        self.source = "amdsmi"

    def _read_amdsmi(self):
        amdsmi, h = self._smi
        out = {}
        try:
            c = amdsmi.amdsmi_get_clock_info(h, amdsmi.AmdSmiClkType.GFX)
            v = c.get("clk", c.get("cur_clk"))
            out["sclk_mhz"] = float(v) if isinstance(v, (int, float)) else None
        except Exception:                                         # noqa: BLE001
            out["sclk_mhz"] = None
        try:
            c = amdsmi.amdsmi_get_clock_info(h, amdsmi.AmdSmiClkType.MEM)
            v = c.get("clk", c.get("cur_clk"))
            out["mclk_mhz"] = float(v) if isinstance(v, (int, float)) else None
        except Exception:                                         # noqa: BLE001
            pass
        try:
            pw = amdsmi.amdsmi_get_power_info(h)
            for k in ("current_socket_power", "average_socket_power"):
                if isinstance(pw.get(k), (int, float)):
                    out["power_w"] = float(pw[k])
                    break
        except Exception:                                         # noqa: BLE001
            pass
        return out

    def read(self):
        if self.source is None:
            return {}
        if self._smi is not None:
            return self._read_amdsmi()
        out = {}
        for k, (path, scale) in self._files.items():
            try:
                out[k] = float(open(path).read()) * scale
            except (OSError, ValueError):
                pass
        return out


def _summ(vals):
    vals = sorted(v for v in vals if v is not None)
    if not vals:
        return None
    return {"median": vals[len(vals) // 2], "min": vals[0], "max": vals[-1], "samples": len(vals)}


def box_state(wl, ctx, ms_per_step, want_ms=250.0):
    """-> dict for `roofline.box`.  (1) The same step queued for ~want_ms more (the clocks and the power of the timed region's
    load, which itself lasts only tens of milliseconds: too short for the sensors' own averaging) while the host polls the
    sensors until the last step's event completes; (2) right after it, grid-stride float4 streams of 512 MiB operands through
    kgcn_hbm_probe in the read : write mixes of the priced kernels (2 : 1 fused backward, 1 : 1 SpMM, read only)."""
    import torch
    from kgcn_amd import _lib
    out = {}
    try:
        sensors = BoxSensors(ctx.device.index or 0)
        n = int(min(2000, max(20, want_ms / max(ms_per_step, 1e-3))))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        samples = []
        e0.record()
        for i in range(n):
            wl.step()
            if i % 8 == 7 and sensors.source:                     # the launch queue is ahead of the device: the GPU is under load here
                samples.append(sensors.read())
        e1.record()
        while sensors.source and not e1.query():
            samples.append(sensors.read())
            time.sleep(0.002)
        torch.cuda.synchronize()
        out["sustained"] = {"steps": n, "ms_per_step": e0.elapsed_time(e1) / n,
                            "sclk_mhz": _summ([x.get("sclk_mhz") for x in samples]),
                            "mclk_mhz": _summ([x.get("mclk_mhz") for x in samples]),
                            "power_w": _summ([x.get("power_w") for x in samples]),
                            "sensors": sensors.source, "sensors_unavailable": None if sensors.source else sensors.why}
    except Exception as e:                                        # noqa: BLE001  (a measurement aid never fails the bench line)
        out["sustained"] = {"error": repr(e)}
    try:
        nbytes = 512 << 20
        a = torch.empty(nbytes // 4, device=ctx.device).fill_(1.0)
        a2 = torch.empty_like(a).fill_(2.0)
        b = torch.empty_like(a)
        moved = {0: 2 * nbytes, 1: 3 * nbytes, 2: nbytes}
        names = {0: "copy_1r1w", 1: "add_2r1w", 2: "read_only"}
        probe = {}
        for mix in (1, 0, 2):
            call = lambda: _lib.check(_lib.lib.kgcn_hbm_probe(mix, _lib.ptr(a), _lib.ptr(a2), _lib.ptr(b), nbytes,
                                                               _lib.current_stream()), "kgcn_hbm_probe")
            for _ in range(3):
                call()
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(41)]
            evs[0].record()
            for k in range(40):
                call()
                evs[k + 1].record()
            torch.cuda.synchronize()
            ms = sorted(evs[k].elapsed_time(evs[k + 1]) for k in range(40))
            probe[names[mix]] = {"GB/s": moved[mix] / (ms[20] * 1e-3) / 1e9, "median_ms": ms[20],
                                 "frac_of_peak": moved[mix] / (ms[20] * 1e-3) / 1e9 / HBM_PEAK_GBS}
        probe["note"] = "kgcn_hbm_probe, 512 MiB per operand (beyond the 256 MiB last-level cache), 40 launches each, right after the sustained loop"
        out["hbm_probe"] = probe
        del a, a2, b
    except Exception as e:                                        # noqa: BLE001
        out["hbm_probe"] = {"error": repr(e)}
    return out


# ---------------------------------------------------------------------------------------------
# CPU baseline: the C restatement (oracle/kgcn_ref.c) on the host cores -- reported, never shipped
# ---------------------------------------------------------------------------------------------
def cpu_baseline(wl, budget_s=12.0, sample=20000):
    from oracle import ref_c
    T = min(sample, wl["csr"].num_graphs)
    off = wl["off"][:T + 1].copy()
    nnz = int(off[-1])
    idx = np.ascontiguousarray(wl["idx"][:nnz])
    val = np.ascontiguousarray(wl["val"][:nnz])
    x = wl["x"][:T].detach().cpu().numpy()
    g = wl["g"][:T].detach().cpu().numpy()
    w = wl["w"].cpu().numpy()
    b = wl["bias"].cpu().numpy()
    threads = ref_c.max_threads()
    ref_c.graphconv_fwd(off, idx, val, x[:256], w, b)       # warm up (page in, spawn threads)
    reps, t0 = 0, time.perf_counter()
    while True:
        ref_c.graphconv_fwd(off, idx, val, x, w, b)
        ref_c.graphconv_bwd(off, idx, val, x, w, g)
        reps += 1
        el = time.perf_counter() - t0
        if el >= budget_s and reps >= 3:
            break
    res = {"value": T * reps / el, "unit": "graphs/sec", "cores": threads, "kind": "port",
           "sample": "%d graphs x %d passes of GraphConv fwd+bwd (oracle/kgcn_ref.c, OpenMP %d "
                     "threads, fp32), %.1f s" % (T, reps, threads, el)}
    # reference-shaped leg: one scipy CSR SpMM and one tiny GEMM per graph, forward and the a-6 / a-7
    # backward, single thread -- the op structure of kgcn/layers.py:107-116, not its TF executor
    import scipy.sparse as sp
    Ts = min(2000, T)
    mats = [sp.csr_matrix((val[off[t]:off[t + 1]], (idx[off[t]:off[t + 1], 0], idx[off[t]:off[t + 1], 1])),
                          shape=(N_NODES, N_NODES)) for t in range(Ts)]
    t0, done = time.perf_counter(), 0
    while time.perf_counter() - t0 < 4.0:
        dw = np.zeros_like(w)
        db = np.zeros((1, w.shape[1]), np.float32)
        for t in range(Ts):
            out = mats[t] @ (x[t] @ w + b)                                        # noqa: F841
            dfw = mats[t].T @ g[t]
            dx = dfw @ w.T                                                        # noqa: F841
            dw += x[t].T @ dfw
            db += dfw.sum(0, keepdims=True)
        done += Ts
    el2 = time.perf_counter() - t0
    res["reference_shaped"] = {"value": done / el2, "unit": "graphs/sec", "cores": 1,
                               "sample": "%d graphs, per-graph scipy.sparse CSR @ (X W + b) + backward, numpy fp32, "
                                         "1 thread, %.1f s" % (done, el2)}
    return res


# ---------------------------------------------------------------------------------------------
# run context
# ---------------------------------------------------------------------------------------------
class Ctx:
    def __init__(self, args):
        import torch
        import torch.distributed as dist
        self.torch, self.dist = torch, dist
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.on_gpu = args.device == "cuda"
        if self.on_gpu:
            if not torch.cuda.is_available():
                raise SystemExit("bench.py needs a GPU (rank %d of %d: the product path has no CPU fallback; "
                                 "--dry --device cpu --backend gloo exercises the launcher and the collective alone)"
                                 % (self.rank, self.world))
            torch.cuda.set_device(self.local_rank)
            self.device = torch.device("cuda", self.local_rank)
        else:
            self.device = torch.device("cpu")
        self.backend = args.backend
        # the data-parallel path (process group, gradient bucket, all-reduce) also runs with ONE rank under a launcher when
        # --force-dist is given: the only way to exercise RCCL inside the captured step on a 1-GPU box
        self.dist_on = self.world > 1 or (args.force_dist and "RANK" in os.environ)
        if self.dist_on:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            kw = {"device_id": self.device} if self.on_gpu else {}
            # the communication libraries print connection banners on fd 1 (gloo always, RCCL with NCCL_DEBUG): stdout
            # is reserved for rank 0's ONE JSON line, so fd 1 points at stderr while the group is being set up
            sys.stdout.flush()
            saved = os.dup(1)
            os.dup2(2, 1)
            try:
                dist.init_process_group(self.backend, rank=self.rank, world_size=self.world, **kw)
                dist.barrier()
            finally:
                sys.stdout.flush()
                os.dup2(saved, 1)
                os.close(saved)

    def sync(self):
        if self.on_gpu:
            self.torch.cuda.synchronize()

    def barrier(self):
        """barrier + device synchronisation on both sides (the contract's bracket of the timed region)."""
        self.sync()
        if self.dist_on:
            self.dist.barrier()
        self.sync()

    def event(self):
        return self.torch.cuda.Event(enable_timing=True) if self.on_gpu else None

    def max_over_ranks(self, x):
        if self.world == 1:
            return x
        t = self.torch.tensor([x], device=self.device, dtype=self.torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def gather_over_ranks(self, x):
        if self.world == 1:
            return [x]
        t = self.torch.tensor([x], device=self.device, dtype=self.torch.float64)
        out = [self.torch.zeros_like(t) for _ in range(self.world)]
        self.dist.all_gather(out, t)
        return [float(o.item()) for o in out]

    def collective_report(self, bucket, weight, in_step_us=None, reps=50):
        """The all-reduce of the gradient bucket alone, event-timed (HIP events on the stream the collective is
        enqueued on; host clock on CPU), after the timed region."""
        if not self.dist_on or bucket is None:
            return None
        torch, dist = self.torch, self.dist
        for p in bucket.params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        for _ in range(5):
            bucket.all_reduce_mean(weight=weight)
        self.barrier()
        if self.on_gpu:
            ev = [(self.event(), self.event()) for _ in range(reps)]
            for a, b in ev:
                a.record()
                bucket.all_reduce_mean(weight=weight)
                b.record()
            self.sync()
            us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
        else:
            us = []
            for _ in range(reps):
                t0 = time.perf_counter()
                bucket.all_reduce_mean(weight=weight)
                us.append((time.perf_counter() - t0) * 1e6)
            us.sort()
        rep = {"ranks": dist.get_world_size(), "backend": dist.get_backend(),
               "what": "one all-reduce (sum) of the flat fp32 gradient bucket per step + pack / scale / unpack launches",
               "bucket_floats": int(bucket.total), "bucket_bytes": int(bucket.total) * 4,
               "allreduce_us_standalone": {"median": us[len(us) // 2], "p10": us[len(us) // 10],
                                           "p90": us[(9 * len(us)) // 10]}}
        if self.on_gpu:
            try:
                rep["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception as e:                                       # noqa: BLE001
                rep["rccl_version"] = "unavailable (%s)" % e
        if in_step_us:
            u = sorted(in_step_us)
            rep["allreduce_us_in_step"] = {"median": u[len(u) // 2], "p10": u[len(u) // 10], "p90": u[(9 * len(u)) // 10]}
        return rep


# ---------------------------------------------------------------------------------------------
# cfg2: one GraphConv layer, forward + backward (the headline)
# ---------------------------------------------------------------------------------------------
def make_cfg2(T, device, seed=1234, normalize=False):
    import torch
    from kgcn_amd import BatchedCSR
    g, r, c = gen_mol_graphs(T, seed=seed)
    val = kipf_values(g, r, c, T, N_NODES) if normalize else np.ones(g.shape[0], np.float32)
    csr = BatchedCSR.from_arrays(g, r, c, val, T, N_NODES, N_NODES, device=device)
    csr.transpose()
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    x = torch.randn((T, N_NODES, FEAT), device=device, dtype=torch.float32, generator=gen)
    grad = torch.randn((T, N_NODES, FEAT), device=device, dtype=torch.float32, generator=gen)
    wrng = np.random.default_rng(4321)                      # identical weights on every rank
    lim = np.sqrt(6.0 / (FEAT + FEAT))
    w = torch.as_tensor(wrng.uniform(-lim, lim, size=(FEAT, FEAT)).astype(np.float32), device=device)
    bias = torch.zeros((1, FEAT), device=device, dtype=torch.float32)
    off = np.zeros(T + 1, np.int64)
    np.cumsum(np.bincount(g, minlength=T), out=off[1:])
    idx = np.stack([r, c], axis=1).astype(np.int32)

    def adjs_of(pick):
        return [[(idx[off[t]:off[t + 1]], val[off[t]:off[t + 1]], [N_NODES, N_NODES])] for t in pick]

    return dict(csr=csr, x=x, g=grad, w=w, bias=bias, off=off, idx=idx, val=val, adjs_of=adjs_of,
                nnz_per_graph=float(g.shape[0]) / T)


class Cfg2:
    name = "cfg2"
    n_events = 5
    keep_outputs = False            # --dump-outputs: set for the last timed step, which then keeps its forward output

    def __init__(self, args, ctx):
        import torch
        from kgcn_amd import layers
        from kgcn_amd.parallel import GradBucket, shard_range, shard_weight
        self.args, self.ctx = args, ctx
        graphs = args.graphs or 100_000
        if args.scaling == "strong":
            lo, hi = shard_range(graphs, ctx.rank, ctx.world)        # contiguous shard of ONE global batch
            self.T, self.T_global = hi - lo, graphs
        else:
            self.T, self.T_global = graphs, graphs * ctx.world
        self.weight = shard_weight(self.T, self.T_global) if ctx.dist_on else None
        self.wl = make_cfg2(self.T, ctx.device, seed=1234 + ctx.rank, normalize=args.normalize)
        self.csr = self.wl["csr"]
        self.layer = layers.GraphConv(FEAT, 1).to(ctx.device)
        self.layer.build((self.T, N_NODES, FEAT), ctx.device)
        with torch.no_grad():
            self.layer.w[0].copy_(self.wl["w"])
            self.layer.bias[0].copy_(self.wl["bias"])
        if args.unfused:
            layers.enabled_batched = True
        self.x = self.wl["x"].requires_grad_(True)
        self.g = self.wl["g"]
        self.bucket = GradBucket(list(self.layer.parameters())) if ctx.dist_on else None
        self.units_local = self.T
        self.units_global = self.T_global

    def setup_passes(self):
        return 25

    def step(self, ev=None):
        self.x.grad = None
        for p in self.layer.parameters():
            p.grad = None
        if ev:
            ev[0].record()
        out = self.layer(self.x, adj=self.csr)
        if ev:
            ev[1].record()
        out.backward(self.g)
        if ev:
            ev[2].record()
        if self.bucket is not None:
            self.bucket.all_reduce_mean(weight=self.weight)
            if ev:
                ev[3].record()
        if self.keep_outputs:
            self.out = out

    def outputs(self):
        """What the last timed step gave its caller: the layer output and dX of a fixed, seeded sample of DUMP_GRAPHS graphs
        (every graph of a smaller batch), dW and dbias."""
        import torch
        pick = np.arange(self.T)
        if self.T > DUMP_GRAPHS:
            pick = np.sort(np.random.default_rng(0).choice(self.T, DUMP_GRAPHS, replace=False))
        sel = torch.as_tensor(pick, device=self.ctx.device)
        return {"output": self.out.detach().index_select(0, sel), "grad_x": self.x.grad.index_select(0, sel),
                "grad_w": self.layer.w[0].grad, "grad_bias": self.layer.bias[0].grad}

    def spmm_probe(self, reps):
        """The batched SpMM alone (the kernel of the north-star 60 % target): forward and adjoint launches on the
        same batch, after the timed region, clocks still in their sustained state."""
        import torch
        from kgcn_amd import ops
        T = self.T
        x2d, g2d = self.wl["x"].detach().reshape(T * N_NODES, FEAT), self.g.reshape(T * N_NODES, FEAT)
        o2d = torch.empty_like(x2d)
        csr_t = self.csr.transpose()
        sev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(max(reps, 20))]
        for _ in range(5):
            ops.bspmm_raw(self.csr, x2d, FEAT, o2d)
            ops.bspmm_raw(csr_t, g2d, FEAT, o2d)
        for e in sev:
            e[0].record()
            ops.bspmm_raw(self.csr, x2d, FEAT, o2d)
            e[1].record()
            ops.bspmm_raw(csr_t, g2d, FEAT, o2d)
            e[2].record()
        torch.cuda.synchronize()
        return [e[0].elapsed_time(e[1]) for e in sev], [e[1].elapsed_time(e[2]) for e in sev]

    def in_step_allreduce_us(self, evs):
        if self.bucket is None:
            return None
        return [e[2].elapsed_time(e[3]) * 1e3 for e in evs]

    def hipgraph_replay(self, steps, warmup):
        """--graph: the same step (forward, backward [, gradient exchange]) captured ONCE in a hipGraph and replayed: at small
        batches (4,096 graphs: example_config batch sizes) the eager step is bound by the host's launch calls, the replay by
        the kernels' own launch latency.  After the timed region of the contract; reported next to `value`, never as it."""
        import torch
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                self.step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        self.x.grad = None
        for p in self.layer.parameters():
            p.grad = None
        from kgcn_amd.train import capture_mode
        with torch.cuda.graph(graph, **capture_mode()):            # (a live process group's watchdog thread must not break the capture)
            self.step()
        for _ in range(max(warmup, 3)):
            graph.replay()
        self.ctx.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            graph.replay()
        self.ctx.barrier()
        dt = self.ctx.max_over_ranks(time.perf_counter() - t0)
        return {"ms_per_step": dt / steps * 1e3, "value": self.units_global * steps / dt, "steps": steps,
                "note": "one hipGraph replay per step (forward + backward%s), same batch" %
                        (" + gradient all-reduce" if self.bucket is not None else "")}

    def report(self, evs):
        """rank 0: config + roofline + cpu_baseline."""
        args, T, wl = self.args, self.T, self.wl
        spmm = self.spmm_probe(args.steps) if (args.full and not args.unfused and not args.profile) else None
        traffic, traffic_stale = {}, None
        tpath = os.path.join(ROOT, "profiles", "traffic_cfg2.json")
        if os.path.exists(tpath) and not args.unfused:
            tj = json.load(open(tpath))
            if tj.get("graphs_per_launch") == T:      # PMC-measured HBM bytes of the same launch shape
                traffic = {k: v.get("bytes") for k, v in tj.items() if isinstance(v, dict)}
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import source_hash                     # comments and white space do not count
                traffic_stale = tj.get("kernel_sources_sha256") != source_hash.sources_sha256(source_hash.CFG2_FILES)
        fwd_st = stats([e[0].elapsed_time(e[1]) for e in evs])
        bwd_st = stats([e[1].elapsed_time(e[2]) for e in evs])
        fwd_ms, bwd_ms = fwd_st["mean_ms"], bwd_st["mean_ms"]
        ab = algorithmic_bytes(N_NODES, FEAT, FEAT, wl["nnz_per_graph"])
        bwd_gbs = ab["bwd"] * T / (bwd_ms * 1e-3) / 1e9
        fwd_gbs = ab["fwd"] * T / (fwd_ms * 1e-3) / 1e9
        spmm_entry = None
        if spmm is not None:
            sb = 2 * 4 * N_NODES * FEAT + ab["csr"]
            sf, sa = stats(spmm[0]), stats(spmm[1])
            spmm_entry = {"kernel": "spmm_slices_kernel<2> (kgcn_bspmm_f32: Bspmm / Bspmdt / Bconv; the two 32-column slices of a graph "
                                    "as waves of one workgroup)", "bound": "hbm",
                          "algorithmic_bytes_per_graph": sb, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                          "forward": dict(sf, achieved=sb * T / (sf["median_ms"] * 1e-3) / 1e9,
                                          frac=sb * T / (sf["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS),
                          "adjoint": dict(sa, achieved=sb * T / (sa["median_ms"] * 1e-3) / 1e9,
                                          frac=sb * T / (sa["median_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS),
                          "traffic": traffic.get("spmm_slices_kernel", traffic.get("spmm_tile_kernel"))}
        config = {"workload": "cfg2: %d random 32-node graphs per GPU (tree+3 edges+self loops, nnz=100), 64-dim "
                              "features, 1 adjacency channel, GraphConv fwd+bwd (dX,dW,dbias)%s"
                              % (T, ", unfused kernels" if args.unfused else ""),
                  "graphs_per_gpu": T, "graphs_global": self.T_global, "n_nodes": N_NODES, "din": FEAT, "dout": FEAT,
                  "nnz_per_graph": wl["nnz_per_graph"], "adjacency_values": "kipf" if args.normalize else "ones"}
        roofline = {"bound": "hbm",
                    "kernel": "dense_wgrad+bspmm (unfused)" if args.unfused else
                              "graphconv_bwd_pairs_kernel (two waves per graph slot; +1 reduce_partials launch, ~5 us, in the event "
                              "bracket)" if T >= 2048 else
                              "graphconv_bwd_planes_kernel (+1 reduce_partials launch, ~5 us, in the event bracket)",
                    "achieved": bwd_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": bwd_gbs / HBM_PEAK_GBS, "traffic": traffic.get("graphconv_bwd_pairs_kernel" if T >= 2048 else "graphconv_bwd_planes_kernel"),
                    "launch_ms": bwd_st,
                    "traffic_note": "HBM bytes per launch, rocprofv3 PMC (profiles/traffic_cfg2.json); "
                                    "algorithmic bytes per launch = %d" % int(ab["bwd"] * T),
                    "traffic_stale": traffic_stale,      # True: the kernel sources changed since that PMC run

                    "algorithmic_bytes_per_graph": ab["bwd"], "avg_launch_ms": bwd_ms,
                    "fwd_kernel": {"achieved": fwd_gbs, "frac": fwd_gbs / HBM_PEAK_GBS,
                                   "algorithmic_bytes_per_graph": ab["fwd"], "avg_launch_ms": fwd_ms,
                                   "launch_ms": fwd_st, "traffic": traffic.get("graphconv_fwd_full_kernel")},
                    "spmm_kernel": spmm_entry,
                    "layer_frac_of_hbm_peak": ab["layer"] * T / ((fwd_ms + bwd_ms) * 1e-3) / 1e9 / HBM_PEAK_GBS}
        extra = {}
        if self.ctx.world == 1 and args.full and not args.no_cpu_baseline and not args.profile:
            extra["cpu_baseline"] = cpu_baseline(wl)
        return config, roofline, extra


# ---------------------------------------------------------------------------------------------
# cfg4 / cfg5: model-level training steps (hipGraph-captured by default)
# ---------------------------------------------------------------------------------------------
def abi_roofline_of(step_fn):
    """Every C-ABI call of ONE eager step bracketed by HIP events and priced with its algorithmic bytes / flops
    (tools/abi_roofline.py); returns the merged rows, largest time first."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_roofline
    rec = abi_roofline.instrument()
    step_fn()                                        # warm (allocator) with the wrappers in place
    torch.cuda.synchronize()
    rec.calls, rec.on = [], True
    step_fn()
    torch.cuda.synchronize()
    rec.on = False
    abi_roofline.restore(rec)
    return rec.rows(), sorted(rec.other)


# kernel behind the dominant call (for `traffic`): (entry prefix, matrix-pipe products) -> kernel name prefix in profiles/traffic_<cfg>.json
_KERNEL_OF = {("kgcn_dense_fwd", 3): "gemmh_fwd_kernel<0", ("kgcn_dense_dx_dact", 3): "gemmh_fwd_kernel<1",
              ("kgcn_dense_wgrad", 3): "gemmh_wgradl_kernel", ("kgcn_dense_bwd", 3): "gemmb_kernel", ("kgcn_dense_fwd", 6): "gemm3_fwd_kernel",
              ("kgcn_dense_wgrad", 6): "gemm3_wgrad_kernel", ("kgcn_bspmm", 0): "spmm_", ("kgcn_bconv", 0): "spmm_",
              ("kgcn_gin_aggregate", 0): "spmm_tile_kernel"}


def kernel_sources_sha256():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import source_hash                                 # every .hip / .h under kgcn_amd/csrc, comments and white space removed
    return source_hash.sources_sha256()


def traffic_of(cfg, entry, products):
    """HBM bytes per launch of the kernel behind `entry` from profiles/traffic_<cfg>.json (rocprofv3 PMC passes of
    tools/profile_config.sh: FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md + WRITE_SIZE), with a flag telling
    whether the kernel sources changed since that profile was taken."""
    path = os.path.join(ROOT, "profiles", "traffic_%s.json" % cfg)
    if not os.path.exists(path):
        return None, None, None
    tj = json.load(open(path))
    pref = next((v for (e, p), v in _KERNEL_OF.items() if entry.startswith(e) and p == products), None)
    if pref is None:
        return None, None, None
    cands = sorted(((k, v) for k, v in tj.get("kernels", {}).items() if k.startswith(pref)), key=lambda kv: -kv[1].get("us_per_step", 0))
    if not cands:
        return None, None, None
    stale = tj.get("kernel_sources_sha256") != kernel_sources_sha256()
    return cands[0][1].get("bytes"), cands[0][0], stale


def roofline_from_rows(rows, unpriced, cfg=None):
    if not rows:
        return {"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None}
    top = next((r for r in rows if not r.get("nominal")), rows[0])     # largest time among the calls with real byte / flop figures
    mfma = top["bound"] == "mfma"
    traffic, kernel, stale = traffic_of(cfg, top["entry"], top["mfma_products"]) if cfg else (None, None, None)
    return {"bound": top["bound"], "kernel": "%s [%s] x%d per step" % (top["entry"], top["shape"], top["calls"]),
            "achieved": top["TFLOP_per_s"] if mfma else top["GB_per_s"],
            "peak": top["mfma_peak_TFLOPs"] if mfma else HBM_PEAK_GBS, "unit": "TFLOP/s" if mfma else "GB/s",
            "frac": top["frac"], "traffic": traffic, "traffic_kernel": kernel, "traffic_stale": stale,
            "peak_note": ("fp32 flops against the dense f16 / bf16 matrix rate 2.5 PF divided by the %d matrix-pipe products the "
                          "kernel spends per fp32 product" % top["mfma_products"]) if mfma and top["mfma_products"] >= 3 else None,
            "avg_launch_ms": top["us"] / top["calls"] * 1e-3,
            "per_call_table": rows, "unpriced_calls": unpriced,
            "method": "one extra EAGER step after the timed region; every C-ABI call priced with the algorithmic bytes / flops of "
                      "its arguments; the GEMMs and aggregations are timed as 8 back-to-back launches inside one HIP-event "
                      "bracket (busy device, warm clocks: within a launch gap of the rocprofv3 duration of the same kernel inside "
                      "the captured step, profiles/r04_*_cfg*_rocprof.txt); bound = the larger of the HBM and matrix-pipe floors "
                      "(tools/abi_roofline.py)"}


def train_exchange(bucket, opt, weight):
    from kgcn_amd import train
    return train._exchange(bucket, opt, weight)


class _ModelStep:
    """Shared by cfg4 / cfg5: eager or hipGraph-captured train step + the per-call roofline of one eager step."""
    n_events = 2
    assemble_in_step = False        # a new mini-batch per step: the device-side assembly is the head of the (captured) step
    keep_outputs = False            # --dump-outputs: set for the last timed step, which then keeps (loss, logits)

    def setup_passes(self):
        return 5

    def _finish(self, model, loss_fn, static_batch, labels, mask, **fwd_kwargs):
        from kgcn_amd import parallel, train
        ctx = self.ctx
        self.model, self.loss_fn, self.sb, self.labels, self.mask, self.kw = model, loss_fn, static_batch, labels, mask, \
            fwd_kwargs
        dp = ctx.dist_on
        self.weight = parallel.shard_weight(self.units_local, self.units_local * ctx.world) if dp else None
        params = list(model.parameters())
        self.opt = train.TFAdam(params, lr=1e-3)
        # the bucket IS the optimiser's flat gradient buffer: pack, all-reduce, fused update -- nothing copied back
        self.bucket = parallel.GradBucket(params, flat=self.opt.flat) if dp else None
        self.graph_step = None
        if not self.args.eager:
            self.graph_step = train.GraphedTrainStep(model, self.opt, loss_fn, static_batch, labels, mask,
                                                     bucket=self.bucket, shard_weight=self.weight,
                                                     capture_assembly=self.assemble_in_step, **fwd_kwargs)

    def _eager_step(self):
        from kgcn_amd import ops
        self.opt.zero_grad(set_to_none=True)
        ops.weight_tables.refresh()
        if self.assemble_in_step:
            self.sb.assemble()
        logits = self.model(self.sb.features, self.sb.adjacency, **self.kw)
        cost_opt, cost_sum = self.loss_fn(logits, self.labels, self.mask)
        with ops.deferred_reductions(root=cost_opt):
            cost_opt.backward()
        self.opt.step(packed=train_exchange(self.bucket, self.opt, self.weight))
        return cost_sum, logits

    def step(self, ev=None):
        if ev:
            ev[0].record()
        self.next_batch()
        if self.graph_step is not None:
            res = self.graph_step.replay()
        else:
            res = self._eager_step()
        if ev:
            ev[1].record()
        if self.keep_outputs:
            self.out = res

    def outputs(self):
        """What the last timed step gave its caller: the loss (GraphedTrainStep's cost_sum), the logits and the parameters
        after the update."""
        cost_sum, logits = self.out
        outs = {"loss": cost_sum.detach().reshape(-1), "logits": logits.detach()}
        outs.update(("param_%02d" % i, p.detach()) for i, p in enumerate(self.opt.params))
        return outs

    def in_step_allreduce_us(self, evs):
        return None

    def model_roofline(self):
        if self.args.profile or not self.args.full:
            return roofline_from_rows([], [])
        rows, unpriced = abi_roofline_of(self._eager_step)
        return roofline_from_rows(rows, unpriced, self.name)


class Cfg4(_ModelStep):
    name = "cfg4"
    assemble_in_step = True

    def __init__(self, args, ctx):
        import torch
        from kgcn_amd import data_util as D, models
        self.args, self.ctx = args, ctx
        N, F, TASKS = 50, 81, 12
        G = args.graphs or 125_000
        B = args.batch or 4096
        dev = ctx.device
        t0 = time.perf_counter()
        sizes, g, r, c, rng = gen_tox21_like(G, N, seed=4 + ctx.rank)         # every rank its own molecules
        chan = D.normalize_adj(D.FlatAdjacency(g, r, c, np.ones(g.shape[0], np.float32), G, N))
        valid = np.arange(N)[None, :] < sizes[:, None]
        feats = rng.standard_normal((G, N, F)).astype(np.float32) * valid[:, :, None]
        labels = (rng.random((G, TASKS)) < 0.3).astype(np.float32)
        mask_label = (rng.random((G, TASKS)) < 0.8).astype(np.float32)
        self.gen_s = time.perf_counter() - t0
        self.rng, self.G, self.B, self.N, self.F = rng, G, B, N, F
        self.mean_valid = float(sizes.mean())
        self.ds = D.DeviceGraphDataset([chan], feats, device=dev, sizes=sizes)
        self.dataset_bytes = int(feats.nbytes + 8 * g.shape[0] + 4 * (G * N + 1))
        self.lab_d, self.ml_d = torch.from_numpy(labels).to(dev), torch.from_numpy(mask_label).to(dev)
        self.sizes_d = torch.from_numpy(sizes.astype(np.int32)).to(dev)
        torch.manual_seed(0)                                                    # the same initial weights on every rank
        model = models.MultitaskGCN(1, TASKS, ragged=not args.padded).to(dev)
        sb = self.ds.static_batch(B) if args.padded else \
            self.ds.static_ragged_batch(B, augmented_features=models.wants_augmented_features(model, F))
        # labels / label mask / true sizes of the batch come out of the same device-side assembly as its adjacency and features
        self.lab_s, self.ml_s, self.en_s = sb.add_table(self.lab_d), sb.add_table(self.ml_d), sb.add_table(self.sizes_d)
        sb.load(np.arange(B))
        self.capacity = getattr(sb, "capacity", B * N)
        model(sb.features, sb.adjacency, enabled_node_nums=self.en_s)           # Keras-style build
        mask = torch.ones(B, device=dev)
        self.units_local, self.units_global = B, B * ctx.world
        self.perm = rng.permutation(G)
        self.cursor = 0
        ml_s = self.ml_s
        self._finish(model, lambda lg, lb, mk: models.masked_sigmoid_ce(lg, lb, mk, ml_s), sb, self.lab_s, mask,
                     enabled_node_nums=self.en_s)

    def next_batch(self):
        """Mini-batch selection (host: a slice of the epoch's permutation, one pinned upload); the assembly itself -- the
        adjacency containers, feature rows, labels, label mask and sizes of the selected graphs -- runs on the device as the
        head of the step."""
        G, B = self.G, self.B
        lo = self.cursor
        if lo + B > G:
            lo = self.cursor = 0
        self.cursor += B
        idx = self.perm[lo:lo + B]
        self.sb.stage(idx)                                # one pinned upload; the assembly kernels are the head of the step

    def report(self, evs):
        args = self.args
        config = {"workload": "cfg4: example_model/model_multitask.py training step (GraphConv 256, 256, GraphDense 256, "
                              "GraphConv 50, BN, GraphDense 50, gather, Dense 12; masked sigmoid CE; TF-Adam), %d "
                              "Tox21-shaped molecules resident per GPU, batch %d per GPU, N=50 padded (true sizes 5..50, "
                              "mean %.1f), F=81, 12 tasks, %s, %s" % (self.G, self.B, self.mean_valid,
                                                                       "all padded rows computed" if args.padded else
                                                                       "valid rows only (ragged-compact)",
                                                                       "eager launches" if args.eager else
                                                                       "one hipGraph per step"),
                  "graphs_resident_per_gpu": self.G, "batch_per_gpu": self.B, "batch_global": self.units_global,
                  "n_nodes_padded": self.N, "mean_valid_nodes": self.mean_valid, "rows_per_step": self.capacity,
                  "features": self.F, "tasks": 12,
                  "dataset_bytes_hbm": self.dataset_bytes, "host_generation_s": round(self.gen_s, 2)}
        return config, self.model_roofline(), {}


class Cfg5(_ModelStep):
    name = "cfg5"

    def __init__(self, args, ctx):
        import types
        import torch
        from kgcn_amd import BatchedAdjacency, BatchedCSR, models
        self.args, self.ctx = args, ctx
        N, D = 10, 256
        B = args.graphs or 20_000
        dev = ctx.device
        g, r, c, lab, rng = gen_ring_graphs(B, N, seed=5 + ctx.rank)
        csr = BatchedCSR.from_arrays(g, r, c, np.ones(g.shape[0], np.float32), B, N, N, device=dev)
        adj = BatchedAdjacency([csr])
        gen = torch.Generator(device=dev)
        gen.manual_seed(5 + ctx.rank)
        x = torch.randn((B, N, D), device=dev, generator=gen)
        labels = torch.nn.functional.one_hot(torch.from_numpy(lab), 2).float().to(dev)
        mask = torch.ones(B, device=dev)
        torch.manual_seed(0)
        model = models.GIN(1, 2, width=D).to(dev)
        model(x, adj)
        self.B, self.nnz = B, int(g.shape[0])
        self.units_local, self.units_global = B, B * ctx.world
        self._finish(model, models.masked_softmax_ce, types.SimpleNamespace(features=x, adjacency=adj), labels, mask)

    def next_batch(self):
        pass                                             # the batch is resident (one fixed batch per GPU)

    def report(self, evs):
        config = {"workload": "cfg5: example_model/model_gin.py training step at width 256 (2 x [GINAggregate, GraphDense "
                              "256 relu x2], gather x2, Dense 2; masked softmax CE; TF-Adam), %d synthetic ring graphs "
                              "(synth_generator_ring.py distribution, N=10) per GPU per step, 256-dim features, %s"
                              % (self.B, "eager launches" if self.args.eager else "one hipGraph per step"),
                  "graphs_per_gpu": self.B, "n_nodes": 10, "features": 256, "nnz_per_graph": self.nnz / self.B}
        return config, self.model_roofline(), {}


class Cfg1(_ModelStep):
    """BASELINE config 1 (example_jbl/synthetic.jbl + example_model/model.py, example_config/synth.json: batch 30): the
    reference's own CPU-runnable training case -- 3 x GraphConv(50), BN, GraphDense(50), gather, Dense(2), masked softmax CE,
    TF-Adam -- on the shipped 200 graphs (tests/golden/g1_synthetic_raw.npz = the converted .jbl), tiled to --graphs graphs
    resident in HBM; one step = one mini-batch of --batch (30) graphs assembled on the device."""
    name = "cfg1"
    assemble_in_step = True

    def __init__(self, args, ctx):
        import torch
        from kgcn_amd import data_util as D, models
        self.args, self.ctx = args, ctx
        z = np.load(os.path.join(ROOT, "tests", "golden", "g1_synthetic_raw.npz"))
        G = args.graphs or 20_000
        rep = -(-G // z["dense_adj"].shape[0])
        dense = np.tile(z["dense_adj"].astype(np.int64), (rep, 1, 1))[:G]
        feats = np.tile(z["feature"], (rep, 1, 1)).astype(np.float32)[:G]
        labels = np.tile(z["label"], (rep, 1)).astype(np.float32)[:G]
        chans, _ = D.build_adjs({"dense_adj": dense, "max_node_num": 10})
        self.ds = D.DeviceGraphDataset(chans, feats, device=ctx.device)
        self.G, self.B = G, args.batch or 30
        B = self.B
        self.lab_d = torch.from_numpy(labels).to(ctx.device)
        self.rng = np.random.default_rng(ctx.rank)
        torch.manual_seed(0)
        model = models.GCN(1, 2).to(ctx.device)
        sb = self.ds.static_batch(B)
        self.lab_s = sb.add_table(self.lab_d)
        sb.load(np.arange(B))
        model(sb.features, sb.adjacency)
        self.units_local, self.units_global = B, B * ctx.world
        self._finish(model, models.masked_softmax_ce, sb, self.lab_s, torch.ones(B, device=ctx.device))

    def next_batch(self):
        idx = self.rng.integers(0, self.G, size=self.B)
        self.sb.stage(idx)                                # the assembly kernels are part of the step (head of the hipGraph)

    def report(self, evs):
        from kgcn_amd import layers
        rows = self.B * 10
        config = {"workload": "cfg1: example_model/model.py training step (3 x GraphConv(50) sigmoid, BN, GraphDense(50), gather, "
                              "Dense(2); masked softmax CE; TF-Adam) on example_jbl/synthetic.jbl (200 graphs of 10 nodes, 3 "
                              "features) tiled to %d graphs resident per GPU, batch %d per GPU assembled on the device, %s, %s"
                              % (self.G, self.B, "cross-layer stack kernels" if layers.stack_fusion and rows <=
                                 layers.stack_fusion_max_rows else "per-layer kernels",
                                 "eager launches" if self.args.eager else "one hipGraph per step"),
                  "graphs_resident_per_gpu": self.G, "batch_per_gpu": self.B, "n_nodes": 10, "features": 3}
        return config, self.model_roofline(), {}


class Cfg3(_ModelStep):
    """BASELINE config 3 (example_config/sparse.json, example_model/sparse.py): the kgcn-sparse path -- ONE block-diagonal
    [sum N x sum N] adjacency per batch of 128 molecules (20..50 atoms), 128-dim features, 3 x GraphConv(256) relu,
    GraphDense(256), BN, per-molecule sum, tanh, Dense(10); summed sparse softmax CE; TF-Adam.  The batch is resident."""
    name = "cfg3"

    def __init__(self, args, ctx):
        import types
        import torch
        from kgcn_amd import data_util as D, models
        self.args, self.ctx = args, ctx
        nmol, F = args.graphs or 128, 128
        rng = np.random.default_rng(3 + ctx.rank)
        size = rng.integers(20, 51, size=nmol)
        rows, cols, elem, deg = [], [], [], []
        for n in size:                                       # random tree + 3 extra edges + self loops per molecule
            a = np.zeros((n, n), np.bool_)
            for i in range(1, n):
                j = rng.integers(0, i)
                a[i, j] = a[j, i] = True
            for _ in range(3):
                i, j = rng.integers(0, n, size=2)
                a[i, j] = a[j, i] = True
            a[np.arange(n), np.arange(n)] = True
            r, c = np.nonzero(a)
            d = a.sum(axis=0)
            rows.append(r); cols.append(c); elem.append(len(r)); deg.append(np.where(r == c, 0, d[r]))
        total = int(size.sum())
        feats = rng.standard_normal((total, F)).astype(np.float32)
        fr = np.concatenate([np.repeat(np.arange(n), F) for n in size])
        fc = np.tile(np.arange(F), total)
        adj_row, adj_col = np.concatenate(rows), np.concatenate(cols)
        batch = D.block_diagonal_batch(size, adj_row, adj_col, np.ones(adj_row.shape[0], np.float32), np.asarray(elem),
                                       np.concatenate(deg), fr, fc, feats.reshape(-1), size * F, F, max_degree=0,
                                       normalize=True, device=ctx.device)
        self.nmol, self.total, self.nnz = nmol, total, int(adj_row.shape[0])
        labels = torch.from_numpy(rng.integers(0, 10, size=nmol)).to(ctx.device)
        torch.manual_seed(0)
        model = models.SparseGCN(10).to(ctx.device)
        model(batch)
        self.units_local, self.units_global = nmol, nmol * ctx.world
        sbn = types.SimpleNamespace(features=batch, adjacency=None)
        self._finish(_SparseAdapter(model), lambda lg, lb, mk: (models.sparse_softmax_ce_sum(lg, lb),) * 2, sbn, labels,
                     torch.ones(nmol, device=ctx.device))

    def next_batch(self):
        pass

    def report(self, evs):
        config = {"workload": "cfg3: example_model/sparse.py training step on the kgcn-sparse path: %d molecules (20..50 atoms) "
                              "as ONE block-diagonal [%d x %d] adjacency (%d stored entries, Kipf-normalised), 128-dim "
                              "features, 3 x GraphConv(256) relu, GraphDense(256), BN, per-molecule sum, tanh, Dense(10); "
                              "summed sparse softmax CE; TF-Adam; %s" % (self.nmol, self.total, self.total, self.nnz,
                                                                        "eager launches" if self.args.eager else
                                                                        "one hipGraph per step"),
                  "molecules_per_gpu": self.nmol, "rows": self.total, "features": 128}
        return config, self.model_roofline(), {}


class _SparseAdapter:
    """models.SparseGCN takes the BlockDiagonalBatch as its only argument; the train-step helpers call
    model(features, adjacency, **kw)."""

    def __init__(self, model):
        self.model = model

    def parameters(self):
        return self.model.parameters()

    def __call__(self, batch, _adjacency=None, **kw):
        return self.model(batch)


# ---------------------------------------------------------------------------------------------
# --dry: the multi-rank path without the kernels (launcher + bucket exchange), any device / backend
# ---------------------------------------------------------------------------------------------
PARAM_SHAPES = {
    "cfg1": [(3, 50), (1, 50), (50, 50), (1, 50), (50, 50), (1, 50), (50,), (50,), (50, 50), (50,), (50, 2), (2,)],
    "cfg2": [(64, 64), (1, 64)],
    "cfg3": [(128, 256), (1, 256), (256, 256), (1, 256), (256, 256), (1, 256), (256, 256), (256,), (256,), (256,), (256, 10),
             (10,)],
    "cfg4": [(81, 256), (1, 256), (256, 256), (1, 256), (256, 256), (256,), (256, 50), (1, 50), (50,), (50,), (50, 50),
             (50,), (50, 12), (12,)],
    "cfg5": [(), (), (256, 256), (256,), (256, 256), (256,), (256, 256), (256,), (256, 256), (256,), (512, 2), (2,)],
}


class Dry:
    n_events = 2

    def __init__(self, args, ctx):
        import torch
        from kgcn_amd.parallel import GradBucket, shard_range, shard_weight
        self.args, self.ctx = args, ctx
        self.name = args.config
        graphs = args.graphs or 1000
        if args.scaling == "strong":
            lo, hi = shard_range(graphs, ctx.rank, ctx.world)
            self.units_local, self.units_global = hi - lo, graphs
        else:
            self.units_local, self.units_global = graphs, graphs * ctx.world
        self.weight = shard_weight(self.units_local, self.units_global) if ctx.dist_on else None
        self.params = [torch.nn.Parameter(torch.zeros(s, device=ctx.device)) for s in PARAM_SHAPES[args.config]]
        self.bucket = GradBucket(self.params) if ctx.dist_on else None
        self.checked = 0

    def setup_passes(self):
        return 1

    def step(self, ev=None):
        torch, ctx = self.ctx.torch, self.ctx
        if ev and ev[0] is not None:
            ev[0].record()
        for i, p in enumerate(self.params):                       # "local mean gradients" of rank r: (r + 1)(i + 1)
            p.grad = torch.full_like(p, float((ctx.rank + 1) * (i + 1)))
        if self.bucket is not None:
            self.bucket.all_reduce_mean(weight=self.weight)
            # sum_r w_r (r + 1)(i + 1) with w_r = B_r / B
            from kgcn_amd.parallel import shard_range
            if self.args.scaling == "strong":
                ws = [(shard_range(self.units_global, r, ctx.world)[1] - shard_range(self.units_global, r, ctx.world)[0])
                      / self.units_global for r in range(ctx.world)]
            else:
                ws = [1.0 / ctx.world] * ctx.world
            want = sum(w * (r + 1) for r, w in enumerate(ws))
            for i, p in enumerate(self.params):
                if not torch.allclose(p.grad, torch.full_like(p, want * (i + 1)), rtol=1e-6, atol=0):
                    raise SystemExit("dry run: rank %d parameter %d: reduced gradient %r != %r"
                                     % (ctx.rank, i, float(p.grad.reshape(-1)[0]), want * (i + 1)))
            self.checked += 1
        if ev and ev[1] is not None:
            ev[1].record()

    def outputs(self):
        return {"grad_%02d" % i: p.grad for i, p in enumerate(self.params)}

    def in_step_allreduce_us(self, evs):
        return None

    def report(self, evs):
        config = {"workload": "DRY RUN of %s: launcher + gradient-bucket exchange only (dummy gradients of the "
                              "configuration's parameter shapes, no kernels); value is NOT a throughput" % self.name,
                  "dry": True, "exchanges_checked": self.checked}
        roofline = {"bound": "hbm", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None}
        return config, roofline, {}


# ---------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", choices=("cfg1", "cfg2", "cfg3", "cfg4", "cfg5"), default="cfg2")
    ap.add_argument("--graphs", type=int, default=0,
                    help="cfg2 / cfg5: graphs per GPU per step (100,000 / 20,000); cfg4: molecules resident per GPU (125,000)")
    ap.add_argument("--batch", type=int, default=0, help="cfg4: molecules per GPU per step (4,096); cfg1: graphs per step (30)")
    ap.add_argument("--normalize", action="store_true", help="cfg2: Kipf-normalised adjacency values")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--unfused", action="store_true", help="cfg2: dense GEMM + Bspmm kernels instead of the fused layer")
    ap.add_argument("--eager", action="store_true", help="cfg4 / cfg5: plain launches instead of one hipGraph per step")
    ap.add_argument("--graph", action="store_true",
                    help="cfg2: additionally capture the step in a hipGraph and report its replay rate as `hipgraph_replay` "
                         "(small batches, e.g. --graphs 4096, are launch-bound in the eager step)")
    ap.add_argument("--padded", action="store_true", help="cfg4: compute all padded rows (round-2 behaviour)")
    ap.add_argument("--side-wgrad", action="store_true",
                    help="A/B switch: weight gradients of the big dense layers on a side stream (measured: no gain, see ops.py)")
    ap.add_argument("--no-wgrad-dact", action="store_true",
                    help="A/B switch: a stand-alone activation-backward pass in front of the first layer's weight gradient")
    ap.add_argument("--contract-first", action="store_true",
                    help="A/B switch: GraphConv always contracts before it aggregates (kgcn_amd.layers.aggregate_first = False)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: --graphs per GPU; strong (cfg2): --graphs in total, sharded over the GPUs")
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl", help="nccl = RCCL on ROCm")
    ap.add_argument("--device", choices=("cuda", "cpu"), default="cuda")
    ap.add_argument("--profile", action="store_true",
                    help="for rocprofv3 runs: nothing after the timed region (no per-call roofline pass, no SpMM probe, no "
                         "CPU baseline), so the trace ends with the timed steps")
    ap.add_argument("--force-dist", action="store_true",
                    help="under a launcher with ONE rank: still build the process group and run the gradient exchange")
    ap.add_argument("--dry", action="store_true",
                    help="launcher + gradient exchange only (no kernels); the only mode that runs without a GPU")
    ap.add_argument("--full", action="store_true",
                    help="also the measurements after the timed region: CPU baseline (cfg2), SpMM probe (cfg2), clocks / power / "
                         "HBM probe (roofline.box), per-call roofline (cfg1 / cfg3 / cfg4 / cfg5)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32, seeded sample of a large output)")
    return ap


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if args.device == "cpu" and not args.dry:
        raise SystemExit("--device cpu needs --dry: the product path has no CPU fallback")
    if args.scaling == "strong" and args.config != "cfg2" and not args.dry:
        raise SystemExit("--scaling strong is defined for cfg2 (cfg4 / cfg5 are fixed per-GPU batches)")
    env_world = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and env_world is None:
        # not under a launcher: spawn one rank per GPU and let rank 0 print the line
        raise SystemExit(self_launch(args.gpus, argv))
    if env_world is not None and int(env_world) != args.gpus:
        raise SystemExit("--gpus %d but the launcher started WORLD_SIZE=%s ranks" % (args.gpus, env_world))

    ctx = Ctx(args)
    torch, dist = ctx.torch, ctx.dist
    if os.environ.get("KGCN_BENCH_FAIL_RANK") == str(ctx.rank):      # test hook (tests/test_bench_launcher.py): a rank that dies
        raise RuntimeError("KGCN_BENCH_FAIL_RANK=%d: this rank fails on purpose" % ctx.rank)
    if args.contract_first:
        from kgcn_amd import layers as _layers
        _layers.aggregate_first = False
    if args.side_wgrad:
        from kgcn_amd import ops as _ops2
        _ops2.side_stream_wgrad = True
    if args.no_wgrad_dact:
        from kgcn_amd import ops as _ops
        _ops.wgrad_dact_fusion = False
    wl = Dry(args, ctx) if args.dry else {"cfg1": Cfg1, "cfg2": Cfg2, "cfg3": Cfg3, "cfg4": Cfg4, "cfg5": Cfg5}[args.config](args, ctx)

    ev = [[ctx.event() for _ in range(wl.n_events)] for _ in range(args.steps)] if ctx.on_gpu else None
    # setup: prime the caching allocator, the lazily built A^T / row-padded containers, the LDS attributes
    # and the clocks (the GPU idles at 107 MHz and needs some tens of milliseconds of load to reach its
    # sustained state, profiles/r01_h_power_clocks.txt) with untimed passes -- part of initialisation, like
    # data generation -- then the W warm-up steps of the contract
    for _ in range(wl.setup_passes()):
        wl.step()
    ctx.sync()
    for _ in range(args.warmup):
        wl.step()
    ctx.barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        if args.dump_outputs and i == args.steps - 1:
            wl.keep_outputs = True
        wl.step(ev[i] if ev else None)
    ctx.barrier()
    local_elapsed = time.perf_counter() - t0
    elapsed = ctx.max_over_ranks(local_elapsed)
    per_rank = ctx.gather_over_ranks(local_elapsed / args.steps * 1e3)
    if args.dump_outputs:
        wl.keep_outputs = False
        if ctx.rank == 0:            # before anything below runs the step again or touches the gradients
            dump_outputs(wl.outputs(), args.dump_outputs)

    box = None
    if ctx.on_gpu and args.full and not args.dry and not args.profile:
        # first thing after the timed region: same load, same clocks.  On EVERY rank: the step holds the gradient all-reduce, and the
        # number of extra steps follows from `elapsed`, the maximum over the ranks -- the same on all of them; rank 0 reports its own GPU
        box = box_state(wl, ctx, elapsed / args.steps * 1e3)

    hipgraph = None
    if args.graph and ctx.on_gpu and args.config == "cfg2" and not args.dry:
        hipgraph = wl.hipgraph_replay(args.steps, args.warmup)
    in_step = wl.in_step_allreduce_us(ev) if ev else None
    collective = ctx.collective_report(getattr(wl, "bucket", None), getattr(wl, "weight", None), in_step)
    if collective is not None:
        collective["per_rank_ms_per_step"] = {"min": min(per_rank), "max": max(per_rank), "all": per_rank}
        collective["env"] = {k: os.environ.get(k) for k in ("HSA_ENABLE_IPC_MODE_LEGACY", "NCCL_DEBUG")}
        # what the exchange costs a step, so that a 1-rank --force-dist run already bounds the N-rank loss: the compute of a rank
        # does not change under WEAK scaling (per-GPU batch fixed), so efficiency ~ compute / (compute + exchange); under STRONG
        # scaling of cfg2 the compute shrinks by N while the exchange does not
        ms = elapsed / args.steps * 1e3
        x_us = (collective.get("allreduce_us_in_step") or collective["allreduce_us_standalone"])["median"]
        compute_ms = max(ms - x_us * 1e-3, 1e-9) if collective.get("allreduce_us_in_step") else ms
        collective["efficiency_expectation"] = {
            "exchange_us": x_us, "exchange_over_step": x_us * 1e-3 / ms,
            "weak": {"at_8_ranks": compute_ms / (compute_ms + x_us * 1e-3),
                     "note": "per-GPU work fixed: the step of N ranks = this rank's compute + one latency-bound all-reduce of the "
                             "same bucket (ring over xGMI: ~2 (N-1) hops of a 16 KB - 1 MB payload)"},
            "strong": {"at_8_ranks": (compute_ms / 8) / (compute_ms / 8 + x_us * 1e-3) if args.config == "cfg2" else None,
                       "note": "cfg2 only (--scaling strong): 1/N of the batch per rank, the exchange stays -- 12,500 graphs per "
                               "rank are ~0.11 ms of kernels against this exchange: the 6x target of north_star is a WEAK-scaling "
                               "target for this path"}}
    if ctx.rank == 0:
        config, roofline, extra = wl.report(ev)
        if box is not None:
            roofline["box"] = box
            pr = box.get("hbm_probe", {})
            mix = "add_2r1w" if args.config == "cfg2" and not args.unfused else "copy_1r1w"
            if roofline.get("achieved") and isinstance(pr.get(mix), dict):
                roofline["frac_of_probe_rate"] = {"value": roofline["achieved"] / pr[mix]["GB/s"], "probe": mix,
                                                  "note": "achieved / what this box's HBM streamed in the kernel's read : write mix"}
            sp = roofline.get("spmm_kernel")
            if sp and isinstance(pr.get("copy_1r1w"), dict):
                sp["forward"]["frac_of_probe_rate"] = sp["forward"]["achieved"] / pr["copy_1r1w"]["GB/s"]
                sp["adjoint"]["frac_of_probe_rate"] = sp["adjoint"]["achieved"] / pr["copy_1r1w"]["GB/s"]
        config["parallelism"] = "dp%d" % ctx.world
        config["collective"] = None if not ctx.dist_on else \
            "one %s all-reduce of the flat gradient bucket (%d floats) per step over %d ranks" \
            % ("RCCL" if ctx.backend == "nccl" else ctx.backend, wl.bucket.total, dist.get_world_size())
        from kgcn_amd import _lib
        config["library"] = {"path": os.path.relpath(_lib.LIB_PATH, ROOT), "dev_overrides": _lib.active_overrides()}
        res = {
            "metric": METRIC if args.config == "cfg2" else "graphs/sec %s training step" % args.config,
            "value": 0.0 if args.dry else wl.units_global * args.steps / elapsed,
            "unit": "graphs/sec",
            "n_gpus": ctx.world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": config,
            "roofline": roofline,
        }
        if collective is not None:
            res["collective"] = collective
        if hipgraph is not None:
            res["hipgraph_replay"] = hipgraph
        res.update(extra)
        print(json.dumps(res), flush=True)
    if ctx.dist_on:
        dist.destroy_process_group()


def _main_tagged():
    """Under a launcher every rank's failure is printed with its rank id before the launcher tears the others down."""
    try:
        main()
    except SystemExit:
        raise
    except BaseException:                                        # noqa: BLE001
        import traceback
        tag = "[bench.py rank %s/%s] " % (os.environ.get("RANK", "0"), os.environ.get("WORLD_SIZE", "1"))
        sys.stderr.write("".join(tag + line + "\n" for line in traceback.format_exc().rstrip().split("\n")))
        sys.stderr.flush()
        raise SystemExit(1)


if __name__ == "__main__":
    _main_tagged()
