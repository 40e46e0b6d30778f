#!/usr/bin/env python3
"""ADNM-UNet training-step benchmark (BASELINE.json metric: training sequences/sec, 5->20 x 128x128).

  python bench.py --gpus N --steps K --warmup W
      N = 1: this process is the one rank.
      N > 1 and no WORLD_SIZE in the environment: this process touches NO GPU, starts N child ranks of itself
             (one per GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set), relays rank 0's JSON
             line and exits with the children's status.
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...
      the driver's form: WORLD_SIZE is set, this process is one rank; --gpus must equal WORLD_SIZE (checked).

One step = forward -> enRainfallLoss -> backward -> (bucketed gradient all-reduce over RCCL, overlapped with backward) ->
clip_grad_norm_ -> AdamW.step -> zero_grad on a synthetic radar batch already resident in HBM (train.py:133-146 of the
reference).  Protocol: W >= 10 warm-up steps, then exactly K timed steps split into up to 5 windows of near-equal
length, each bracketed by barrier + torch.cuda.synchronize() on both sides and reduced with MAX over ranks; `value` /
`ms_per_step` come from the MEDIAN window's time per step, every window is listed in `windows_ms_per_step`.  Rank 0 prints ONE
JSON line.

A plain run does only that: set up, warm up, time the K steps, write --dump-outputs if asked, print the line (`roofline` and
`cpu_baseline` are null there).  --full adds everything else below, after the timed steps: the instrumented steps behind
`roofline` / `families_top` / --dump-prof, the PMC traffic join, `cpu_baseline` and the side file of full tables (--dump-json).

--dump-outputs DIR: what the timed path computed in its last step, as .npy files (write_outputs()).  Inputs and parameters come
from fixed recipes, so two builds run with the same arguments can be compared output for output.

`roofline`: per-kernel HIP-event timing recorded by libadnm_hip around each of its launches (adnm_prof_enable/collect), on the
stream the kernels run on, during extra eagerly-launched steps after the timed region.  The reported kernel is the one with
the largest AGGREGATE time over the library's kernels; `families` lists every north-star kernel family (K1 SSD reduction,
depthwise stencils, wavelet transform, row norms, MFMA GEMMs, dense convs, optimiser) the same way.  `traffic` is the
PMC-measured HBM bytes of that kernel from profiles/pmc_traffic.json — used only if that file was made from the same
kernel sources (hash of csrc/), else null.  `cpu_baseline` times the oracle (oracle/adnm_oracle.py, the CPU restatement of
the reference's algorithm) on the host cores for the same workload, rank 0 / N=1 only.
"""
import argparse
import ctypes
import hashlib
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6.3 TB/s is the measured copy ceiling
N_WINDOWS = 5
OUT_SAMPLE = 1 << 23   # parameter elements --dump-outputs writes at most (32 MB of float32); a fixed, seeded sample above that

# profiler scope (csrc/*.hip ADNM_PROF names) -> north-star kernel family
FAMILIES = [
    ("K1 ssd reduction fwd (kv + apply[+LayerNorm])", ("ssd_kv", "ssd_apply", "ssd_apply_ln")),
    ("K1 ssd reduction bwd (dkv + bwd)", ("ssd_dkv", "ssd_bwd")),
    ("K4 depthwise 3x3 stencil", ("dwconv_k3",)),
    ("K3 depthwise 5x5 stencil (WTConv)", ("dwconv_k5",)),
    ("K3/K4 depthwise weight gradient", ("dwconv_wgrad_k3", "dwconv_wgrad_k5")),
    ("K3 Haar DWT/IDWT (+ the fused WTConv level: DWT + 5x5 stencil)", ("haar_dwt", "haar_idwt", "wt_level")),
    ("K2/K7 row norms (+ the fused residual mix + norm)", ("rownorm_fwd", "rownorm_bwd", "mixnorm_fwd", "mixnorm_bwd")),
    ("K8 instance norm", ("instnorm_stats", "instnorm_apply", "instnorm_bwd_stats", "instnorm_bwd_apply")),
    ("K6 tall-skinny MFMA GEMM", ("tsgemm_nt", "tsgemm_tn")),
    ("K6b short MFMA GEMM", ("skgemm_nt", "skgemm_nn", "skgemm_tn")),
    ("K5 dense 3x3 conv (MFMA implicit GEMM)", ("conv3_fwd", "conv3_dgrad", "conv3_wgrad", "conv3_join")),
    ("K9 transposed conv gathers (its GEMMs are in K6b)", ("convt_col2im", "convt_im2col")),
    ("second-stage folds (batched + critical-path)", ("fold_batch", "skgemm_fold", "ssd_fold", "ssd_bc_fold", "ssd_head_fold", "lincomb_bwd_fold",
                                                      "mixnorm_bwd_fold", "igate_bwd_fold", "bridge_heads_fold", "bridge_pool_fold", "rainloss_fold", "grad_sumsq_fold", "dwconv_wgrad_fold",
                                                      "rownorm_bwd_fold", "tsgemm_tn_fold", "conv3_wgrad_fold", "catmix_bwd_fold", "colsum",
                                                      "adn_prep_bwd_fold", "skip_vec_fold", "skip_scal_fold", "skip_wgrad_fold", "instnorm_bwd_scalar", "swish_bwd_fold")),
    ("scalar/gamma mixes + gates", ("lincomb_fwd", "lincomb_bwd", "catmix_fwd", "catmix_bwd", "gate_fwd", "gate_bwd", "igate_fwd", "igate_bwd", "emul_fwd", "emul_bwd")),
    ("skip-connection gating (EncoderToDecoder core, bridge pools / heads)", ("skip_pool_fwd", "skip_branch_fwd", "skip_branch_bwd", "skip_conv_bwd", "skip_pool_bwd",
                                                                            "bridge_pool_fwd", "bridge_pool_bwd", "bridge_heads_fwd", "bridge_heads_bwd")),
    ("K12 optimiser (sumsq + AdamW)", ("grad_sumsq", "adamw_update")),
]


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps in all (split into up to 5 windows)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure what the headline does not need: the instrumented per-kernel steps "
                         "(roofline, families, --dump-prof), the PMC traffic join, the CPU baseline and the --dump-json side file")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the timed path computed in its last step to DIR/<name>.npy (loss, grad_norm, params)")
    ap.add_argument("--batch", type=int, default=4, help="per-GPU batch (BASELINE config 2: 4)")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--in-frames", type=int, default=5)
    ap.add_argument("--out-frames", type=int, default=20)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--cpu-steps", type=int, default=8, help="timed oracle steps of the CPU baseline of --full (~1.5 s each on 16 threads: ~12-15 s in all)")
    ap.add_argument("--prof-steps", type=int, default=3, help="instrumented steps of --full")
    ap.add_argument("--overlap", type=int, default=-1,
                    help="gradient all-reduce overlapped with backward in bucket order (N>1): 1 on, 0 one blocking all-reduce after "
                         "backward, -1 (default) = on whenever N>1")
    ap.add_argument("--stages", type=int, default=0, help="stage cuts of the overlapped backward: 0 = every stage the model offers (5), 2 = encoder | rest")
    ap.add_argument("--reduce-dtype", default="f32", choices=["f32", "bf16"], help="wire dtype of the gradient all-reduce (N>1)")
    ap.add_argument("--dump-json", default=None,
                    help="--full: side file for the full record (the stdout line + the complete per-family / per-kernel tables); "
                         "default bench_tables.json in the repository root")
    ap.add_argument("--dump-prof", default="", help="--full: write the per-(kernel, shape) HIP-event table of the instrumented steps to this file")
    ap.add_argument("--side-stream", type=int, default=-1,
                    help="weight-gradient leaves (grouped weight-gradient GEMMs / stencils, their folds, the parameter-prep backward nodes) on a second "
                         "stream beside the input-gradient chain = parallel branches of the captured graph: 1 on, 0 off, -1 the trainer's default")
    ap.add_argument("--graph", type=int, default=1, help="1 (default): replay fwd+bwd as captured hipGraphs; 0: eager launches")
    ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16", "fp8"],
                    help="matrix-core precision of the GEMM-shaped kernels.  bf16 (default) = BASELINE config 2's precision: bf16 MFMA operands, "
                         "fp32 accumulation, fp32 master parameters and activations (parity: rel-L2 <= 6e-2 vs the fp32 reference fixtures, <= 3e-2 "
                         "vs the fp32 HIP path, tests/test_model_gpu.py::test_visionmamba_bf16_mfma_vs_reference); f32 = exact fp32 MFMA (the "
                         "bit-level parity path, tolerance 1e-4 / 1e-3); fp8 = BASELINE config 5: per-tensor scaled OCP e4m3 / e5m2 operands into the "
                         "fp8 MFMA for the forward and input-gradient GEMMs / dense convs (delayed scaling, re-calibrated every 16 steps on the "
                         "device), bf16 operands for the weight gradients (parity: rel-L2 <= 1.5e-1, 50-step loss curve within 5 %%, "
                         "tests/test_model_gpu.py::test_visionmamba_fp8_vs_reference)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full and (args.dump_json or args.dump_prof):
        ap.error("--dump-json and --dump-prof come from the measurements of --full: add --full")
    if args.full and args.dump_json is None:
        args.dump_json = os.path.join(ROOT, "bench_tables.json")
    return args


# ------------------------------------------------------------------------------------------------ multi-GPU entry
def spawn_ranks(args):
    """`python bench.py --gpus N` outside a launcher: start N ranks of this script as fresh child processes and SUPERVISE them.
    The parent never initialises HIP (a process that has may not exec/fork GPU children safely, and must not hold a context on
    device 0).  All children are polled: the first one that exits non-zero (import error, device fault, a missing device) takes the
    others down with it — terminate(), then kill() after a grace period — because its peers would otherwise wait in RCCL for ever;
    that rank's stderr tail is printed and the parent exits non-zero.  An overall time limit (ADNM_BENCH_TIMEOUT, default 1500 s)
    bounds the whole job.  Rendezvous: the parent binds port 0 to get a free port and hands it to the children; a rank that cannot
    bind it fails within the init_process_group timeout and is reported like any other failing rank."""
    import tempfile
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    limit = float(os.environ.get("ADNM_BENCH_TIMEOUT", "1500"))
    procs, logs = [], []
    out0 = tempfile.TemporaryFile()
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        if os.environ.get("ADNM_PIN_DEVICES") == "1":   # one visible device per rank (what an unmodified train.py needs)
            env["HIP_VISIBLE_DEVICES"], env["LOCAL_RANK"] = str(r), "0"
        err = tempfile.TemporaryFile()
        logs.append(err)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=out0 if r == 0 else subprocess.DEVNULL, stderr=err))

    def tail(f, n=3000):
        f.seek(0, os.SEEK_END)
        size = f.tell()
        f.seek(max(0, size - n))
        return f.read().decode(errors="replace")

    def stop_all():
        for p in procs:
            if p.poll() is None:
                p.terminate()
        t_end = time.time() + 10.0
        for p in procs:
            try:
                p.wait(timeout=max(0.1, t_end - time.time()))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()

    t0, failed, shown = time.time(), None, [0] * len(procs)
    while True:
        rcs = [p.poll() for p in procs]
        f0 = logs[0]   # relay rank 0's progress lines as they come (the driver watches for output)
        f0.seek(shown[0])
        chunk = f0.read()
        if chunk:
            shown[0] += len(chunk)
            sys.stderr.write(chunk.decode(errors="replace"))
            sys.stderr.flush()
        bad = [r for r, rc in enumerate(rcs) if rc not in (None, 0)]
        if bad:
            failed = (bad[0], rcs[bad[0]])
            break
        if all(rc == 0 for rc in rcs):
            break
        if time.time() - t0 > limit:
            failed = (-1, 124)
            break
        time.sleep(0.2)
    if failed is not None:
        stop_all()
        r, rc = failed
        if r < 0:
            print(f"[bench] the {args.gpus}-rank job exceeded {limit:.0f} s and was stopped", file=sys.stderr)
        else:
            print(f"[bench] rank {r} exited with status {rc}; the other ranks were stopped.  Its stderr tail:", file=sys.stderr)
            if r != 0:
                print(tail(logs[r]), file=sys.stderr)
        sys.stderr.flush()
        return abs(rc) or 1
    out0.seek(0)
    sys.stdout.write(out0.read().decode())
    sys.stdout.flush()
    return 0


# ------------------------------------------------------------------------------------------------ profiler table
def collect_profile(lib):
    buf = ctypes.create_string_buffer(1 << 20)  # one call: collecting also clears the records
    lib.query("adnm_prof_collect", buf, len(buf))
    rows = {}  # key "kernel@bytes_per_launch": one entry per kernel AND shape
    for line in buf.value.decode().splitlines():
        name, cnt, ms, nbytes = line.split("\t")
        rows[name] = {"launches": int(cnt), "ms": float(ms), "bytes": float(nbytes)}
    return rows


def by_kernel(rows):
    out = {}
    for key, r in rows.items():
        a = out.setdefault(key.split("@")[0], {"launches": 0, "ms": 0.0, "bytes": 0.0})
        for f in ("launches", "ms", "bytes"):
            a[f] += r[f]
    return out


def csrc_hash():
    h = hashlib.sha256()
    d = os.path.join(ROOT, "adnm-unet_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h", ".inc")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def pmc_table():
    """profiles/pmc_traffic.json: {"csrc_hash": ..., "commit": ..., "kernels": {scope: {"hbm_bytes_per_step": ...,
    "launches_per_step": ...}}} made by tools/pmc_traffic.py from two rocprofv3 --pmc passes of this command.  Only trusted for
    the kernel sources it was measured on."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(path):
        return None, "no committed PMC pass"
    with open(path) as f:
        t = json.load(f)
    if t.get("csrc_hash") != csrc_hash():
        return None, f"profiles/pmc_traffic.json was measured on other kernel sources (csrc hash {t.get('csrc_hash')}), not used"
    return t, f"profiles/pmc_traffic.json (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE; commit {t.get('commit')})"


def host_cores():
    """CPU threads this process may really use: affinity mask, cgroup quota, and the 16-per-GPU share of the box."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, min(n, int(os.environ.get("ADNM_CPU_THREADS", "16"))))


def cpu_baseline(args, steps):
    """The oracle's full training step on the host CPU (kind 'port': the reference's Python cannot travel)."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import adnm_oracle as O
    from adnm_hip import recipe
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_manifest.json")) as f:
        manifest = json.load(f)
    if (args.in_frames, args.out_frames) != (5, 20):
        return None
    cores = host_cores()
    torch.set_num_threads(cores)
    print(f"[bench] cpu_baseline: oracle on {cores} host threads ...", file=sys.stderr, flush=True)
    sd = recipe.state_dict_from_manifest(manifest)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if manifest[k]["trainable"]}
    full = dict(sd)
    full.update(params)
    opt = torch.optim.AdamW(list(params.values()), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2)
    frames = recipe.radar_batch(args.batch, args.in_frames + args.out_frames, args.size, name="bench")
    x, tgt = frames[:, :args.in_frames], frames[:, args.in_frames:]
    times = []
    for i in range(steps + 1):
        t0 = time.perf_counter()
        out = O.vision_mamba(full, x)
        loss = O.en_rainfall_loss(out, tgt)
        loss.backward()
        torch.nn.utils.clip_grad_norm_([p for p in params.values() if p.grad is not None], 0.025)
        opt.step()
        opt.zero_grad(set_to_none=True)
        times.append(time.perf_counter() - t0)
        print(f"[bench] cpu_baseline step {i}: {times[-1]:.2f} s", file=sys.stderr, flush=True)
    t = sorted(times[1:])[len(times[1:]) // 2]
    return {"value": args.batch / t, "unit": "sequences/s", "cores": cores, "kind": "port",
            "sample": f"{steps} timed full training steps (+1 warm-up) of the oracle at B={args.batch}, {args.size}x{args.size}, fp32, "
                      f"torch.set_num_threads({cores}); median {t:.2f} s/step"}


def summarise(prof, ps, pmc, pmc_src, step_s, prof_step_ms):
    """Per-kernel / per-family tables and the `roofline` object from the profiler rows of `ps` instrumented steps.
    Pure host arithmetic (tests/test_host_logic.py drives it with a canned profile)."""
    agg = by_kernel(prof)
    total_ms = sum(r["ms"] for r in prof.values()) or 1.0

    def line(names):
        """aggregate over profiler scopes: per-step launches / ms / algorithmic bytes, achieved GB/s, fraction of the HBM peak,
        PMC traffic per step and its ratio to the algorithmic bytes (None without a matching PMC pass)"""
        rs = [agg[n] for n in names if n in agg]
        if not rs:
            return None
        ms, by, ln = sum(r["ms"] for r in rs) / ps, sum(r["bytes"] for r in rs) / ps, sum(r["launches"] for r in rs) / ps
        ach = by / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        tr = None
        if pmc:
            # a PMC row is keyed by profiler scope, or by "a|b|c" when one kernel symbol serves several scopes (conv3 fwd/dgrad, the
            # shared fold kernel): such a row counts only when ALL of its scopes are asked for together
            left, tr = {n for n in names if n in agg}, 0.0
            for key, row in pmc["kernels"].items():
                members = set(key.split("|"))
                if members & left:
                    if not members <= set(names):
                        tr = None
                        break
                    tr += row["hbm_bytes_per_step"]
                    left -= members
            if left:
                tr = None
        return {"launches_per_step": round(ln, 1), "ms_per_step": round(ms, 4), "algorithmic_MB_per_step": round(by / 1e6, 2),
                "GBps": round(ach, 1), "frac": round(ach / HBM_PEAK_GBS, 4), "traffic_MB_per_step": None if tr is None else round(tr / 1e6, 2),
                "traffic_over_algorithmic": None if tr is None or by <= 0 else round(tr / by, 3)}

    kernels = {n: line((n,)) for n, _ in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])}
    families = {fam: line(names) for fam, names in FAMILIES if line(names)}
    roofline = None
    if agg:
        # the dominant kernel = the library kernel with the largest AGGREGATE time per step (all its shapes together)
        name = max(agg.items(), key=lambda kv: kv[1]["ms"])[0]
        r, k = agg[name], kernels[name]
        per_launch_bytes = r["bytes"] / r["launches"]
        avg_us = 1e3 * r["ms"] / r["launches"]
        roofline = {"kernel": name, "bound": "hbm", "achieved": k["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": k["frac"],
                    "traffic": None if k["traffic_MB_per_step"] is None else round(1e6 * k["traffic_MB_per_step"] / k["launches_per_step"]),
                    "traffic_source": pmc_src, "launches_per_step": k["launches_per_step"], "avg_launch_us": round(avg_us, 2),
                    "algorithmic_bytes_per_launch": round(per_launch_bytes),
                    "definition": "achieved = algorithmic bytes of this kernel's launches in a step / their HIP-event durations",
                    "hip_kernels_ms_per_step": round(total_ms / ps, 3), "instrumented_step_ms": round(prof_step_ms, 3),
                    "whole_step_frac": round(sum(r_["bytes"] for r_ in agg.values()) / ps / step_s / 1e9 / HBM_PEAK_GBS, 4)}
    return kernels, families, roofline


MAX_LINE = 4000   # the driver parses ONE stdout line; round 3's 20 kB line came back unparsed


def stdout_line(res, families, tables_path):
    """The one JSON line for stdout: the contract's keys, `roofline`, `cpu_baseline` and the 8 families with the most time, held under
    MAX_LINE bytes (families are dropped from the tail if a long path or message would push it over).  The full per-kernel and
    per-family tables go to `tables_path` and stderr."""
    top = sorted(families.items(), key=lambda kv: -kv[1]["ms_per_step"])[:8]
    short = [{"family": f.split(" (")[0], "launches": r["launches_per_step"], "ms": r["ms_per_step"], "frac": r["frac"],
              "traffic_x": r["traffic_over_algorithmic"]} for f, r in top]
    out = dict(res)
    out["tables"] = tables_path
    while True:
        out["families_top"] = short
        s = json.dumps(out, separators=(",", ":"))
        if len(s) < MAX_LINE or not short:
            break
        short = short[:-1]
    if len(s) >= MAX_LINE:
        raise RuntimeError(f"bench.py: the result line is {len(s)} bytes, over the {MAX_LINE}-byte limit")
    return s


def window_sizes(steps):
    """The `steps` timed steps as up to N_WINDOWS windows of near-equal length (the longer ones first); they add up to `steps`."""
    n = min(N_WINDOWS, steps)
    return [steps // n + (i < steps % n) for i in range(n)]


def write_outputs(path, loss, grad_norm, params):
    """--dump-outputs: what the timed path hands its caller after its last step, as .npy files under `path`:
      loss.npy       float64 [1]  the step's enRainfallLoss
      grad_norm.npy  float64 [1]  the total gradient norm before clipping (FlatTrainer.grad_norm())
      params.npy     float32 [n]  the parameters after the step's AdamW update: every tensor of `params` in logical shape, flattened
                                  and concatenated in order; above OUT_SAMPLE elements, the elements at OUT_SAMPLE sorted distinct
                                  indices drawn by a generator seeded with 0 (the same for every run of the same model)
    Returns {name: shape}."""
    import numpy as np
    import torch
    flat = torch.cat([p.detach().reshape(-1).float() for p in params])
    if flat.numel() > OUT_SAMPLE:
        idx = np.sort(np.random.default_rng(0).choice(flat.numel(), OUT_SAMPLE, replace=False, shuffle=False))
        flat = flat[torch.from_numpy(idx).to(flat.device)]
    arrays = {"loss": np.array([float(loss)], dtype=np.float64), "grad_norm": np.array([float(grad_norm)], dtype=np.float64),
              "params": flat.cpu().numpy().astype(np.float32)}
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


# ------------------------------------------------------------------------------------------------ one rank
def main():
    args = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        raise SystemExit(spawn_ranks(args))
    world = int(env_world or "1")
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: start it as `python bench.py --gpus N` (it launches its own "
                         f"ranks) or under torch.distributed.run with --nproc-per-node equal to --gpus")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))

    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    backend = os.environ.get("ADNM_DIST_BACKEND", "nccl")  # "nccl" IS RCCL on ROCm; gloo = the 1-GPU-box rehearsal of the N>1 flow
    ndev = torch.cuda.device_count()
    if world > 1 and backend == "nccl" and local >= ndev:
        raise SystemExit(f"bench.py: rank {rank} wants device {local} but only {ndev} are visible")
    local = local % ndev
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        import datetime
        tmo = datetime.timedelta(seconds=float(os.environ.get("ADNM_DIST_TIMEOUT", "300")))   # a missing peer raises instead of hanging
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=tmo)
        else:
            dist.init_process_group(backend, timeout=tmo)
        assert dist.get_world_size() == world

    from adnm_hip import lib, recipe
    from adnm_hip.trainer import FlatTrainer
    from models.ADNMUNet import create_ADNMUNet
    from models.loss import enRainfallLoss
    lib.load()
    from adnm_hip import ops
    ops.set_mfma_precision(args.dtype)

    os.environ["ADNM_AUTO_DDP"] = "0"   # FlatTrainer owns the gradient collective here (the factory's hook-driven DDP is for train.py)
    model = create_ADNMUNet(args.in_frames, args.out_frames, 6, img_size=args.size)
    recipe.fill_parameters(model)  # identical replicas on every rank, same parameters as the parity fixtures
    model = model.to(dev).train()
    criterion = enRainfallLoss(omega_t=0.57, alpha=0.25, gamma=0.).to(dev)  # train_untils.py:43
    overlap = (world > 1) if args.overlap < 0 else bool(args.overlap)
    # AdamW recipe of train_untils.py:35-42; clip threshold = norm_max of the warm-up epochs (train.py:87,122-124)
    trainer = FlatTrainer(model, criterion, lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                          use_graph=bool(args.graph), overlap=overlap, reduce_dtype=args.reduce_dtype, nstages=args.stages or None,
                          **({} if args.side_stream < 0 else {"side_stream": bool(args.side_stream)}))
    frames = recipe.radar_batch(args.batch, args.in_frames + args.out_frames, args.size, salt=rank, name="bench").to(dev)
    x, tgt = frames[:, :args.in_frames].contiguous(), frames[:, args.in_frames:].contiguous()
    trainer.prepare(x, tgt)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        trainer.step(x, tgt)
    sync()
    if rank == 0:
        print("[bench] warm-up done, timing ...", file=sys.stderr, flush=True)
    sizes = window_sizes(args.steps)
    windows = []   # ms per step of each window
    for w, k in enumerate(sizes):
        sync()
        t0 = time.perf_counter()
        for _ in range(k):
            loss = trainer.step(x, tgt)
        sync()
        dt = time.perf_counter() - t0
        if world > 1:
            tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = float(tmax)
        windows.append(1e3 * dt / k)
        if rank == 0:
            print(f"[bench] window {w}: {windows[-1]:.3f} ms/step over {k} steps", file=sys.stderr, flush=True)
    step_s = 1e-3 * statistics.median(windows)
    loss_val = float(loss.detach())
    if rank == 0 and args.dump_outputs:
        shapes = write_outputs(args.dump_outputs, loss_val, trainer.grad_norm(), list(model.parameters()))
        print(f"[bench] outputs of the last timed step written to {args.dump_outputs}: {shapes}", file=sys.stderr, flush=True)

    def eager_step():  # same work, launched eagerly: per-launch HIP events cannot be recorded inside a graph replay
        return trainer.step(x, tgt, eager=True)

    # ---- --full: instrumented steps (outside the timed region): per-kernel HIP-event timing inside libadnm_hip
    prof = {}
    if args.full and rank != 0 and args.prof_steps > 0:
        for _ in range(args.prof_steps):
            eager_step()  # every rank takes part: the step contains the gradient all-reduce
        torch.cuda.synchronize()
    if args.full and rank == 0 and args.prof_steps > 0:
        lib.query("adnm_prof_enable", 1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.prof_steps):
            eager_step()
        e1.record()
        torch.cuda.synchronize()
        lib.query("adnm_prof_enable", 0)
        prof = collect_profile(lib)
        prof_step_ms = e0.elapsed_time(e1) / args.prof_steps
    if world > 1:
        dist.barrier()

    if rank == 0:
        ps = max(args.prof_steps, 1)
        if args.dump_prof:
            with open(args.dump_prof, "w") as f:
                f.write("kernel@bytes_per_launch\tlaunches_per_step\tavg_us\tms_per_step\tGB/s\n")
                for key, r in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]):
                    f.write(f"{key}\t{r['launches'] / ps:.1f}\t{1e3 * r['ms'] / r['launches']:.2f}\t{r['ms'] / ps:.4f}\t"
                            f"{r['bytes'] / max(r['ms'], 1e-9) / 1e6:.1f}\n")
        kernels, families, roofline = {}, {}, None
        if args.full:
            pmc, pmc_src = pmc_table()
            kernels, families, roofline = summarise(prof, ps, pmc, pmc_src, step_s, prof_step_ms if prof else 0.0)
        res = {
            "metric": f"sequences/sec training ADNM-UNet {args.in_frames}->{args.out_frames}x{args.size}x{args.size}", "value": round(world * args.batch / step_s, 3),
            "unit": "sequences/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "full": args.full,
            "ms_per_step": round(1e3 * step_s, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype,
            "dtype_detail": {"f32": "exact fp32 MFMA (v_mfma_f32_16x16x4_f32) everywhere: the bit-level parity path",
                             "bf16": "bf16 x bf16 -> fp32 on v_mfma_f32_16x16x32_bf16 in every GEMM-shaped kernel; fp32 accumulation, master "
                                     "parameters and every other kernel",
                             "fp8": "config 5: per-tensor scaled OCP e4m3 / e5m2 operands on v_mfma_f32_16x16x32_{fp8,bf8}_fp8, delayed scaling; "
                                    "exemptions in DESIGN.md 3a"}[args.dtype],
            "data": "synthetic",
            "config": {"workload": f"ADNM-UNet create_ADNMUNet({args.in_frames},{args.out_frames},6) {args.size}x{args.size} full training step "
                                   "(fwd + enRainfallLoss + bwd + clip_grad_norm_ + AdamW), recipe parameters, synthetic radar frames in HBM",
                       "per_gpu_batch": args.batch, "global_batch": world * args.batch, "frames": f"{args.in_frames}->{args.out_frames}",
                       "parallelism": f"dp{world}" if world > 1 else "single",
                       "launch": ("hipGraph replay" if args.graph else "eager") + (
                           f", {len(trainer.buckets)} gradient buckets all-reduced ({args.reduce_dtype}) beside backward" if world > 1 and overlap
                           else (", one all-reduce after backward" if world > 1 else "")),
                       "dist_backend": (backend + ("=RCCL" if backend == "nccl" else "")) if world > 1 else None,
                       "protocol": f"{args.warmup} warm-up steps, {args.steps} timed steps in {len(sizes)} windows of {'/'.join(map(str, sizes))}, "
                                   "median window, barrier+sync at window edges, max over ranks",
                       "loss": round(loss_val, 6)},
            "windows_ms_per_step": [round(w, 3) for w in windows],
            "roofline": roofline,
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(args, args.cpu_steps)
        else:
            res["cpu_baseline"] = None
        tables_path = None
        if args.full:
            tables = {"families": families, "kernels": kernels}
            tables_path = args.dump_json
            try:
                with open(tables_path, "w") as f:
                    json.dump(dict(res, **tables), f, indent=1)
            except OSError as e:   # a read-only checkout must not cost the measurement
                print(f"[bench] could not write {tables_path}: {e}", file=sys.stderr)
                tables_path = None
            print("[bench] tables " + json.dumps(tables), file=sys.stderr, flush=True)
        print(stdout_line(res, families, tables_path and os.path.basename(tables_path)), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
