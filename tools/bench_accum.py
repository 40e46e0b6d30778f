#!/usr/bin/env python3
"""One line for the record: gradient accumulation on bench.py's workload (ADNM-UNet 5 -> 20, recipe batch "bench"), FlatTrainer hipGraph
replay with accum_steps = K — ms per optimiser cycle and per micro-step (cycle / K, the last micro-step with its optimiser pass included;
median of 3 windows) and the library's launches of a first, a middle and the last micro-step (counted by adnm_prof_* over eagerly
launched steps).  bench.py measures the plain step and has no accumulation switch.
Run on the GPU box: python tools/bench_accum.py [--accum 8 --batch 4 --size 128 --dtype bf16 --cycles 5 --warmup 2]"""
import argparse, ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import torch
from adnm_hip import ops, lib, recipe
from adnm_hip.trainer import FlatTrainer
from models.ADNMUNet import create_ADNMUNet
from models.loss import enRainfallLoss

ap = argparse.ArgumentParser()
ap.add_argument("--accum", type=int, default=8, help="micro-steps per optimiser step")
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--batch", type=int, default=4, help="micro-batch")
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16", "fp8"])
ap.add_argument("--cycles", type=int, default=5, help="timed optimiser cycles per window (3 windows)")
ap.add_argument("--warmup", type=int, default=2, help="warm-up cycles")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_accum.py: no GPU (a timing without one would mean nothing)")
if args.accum < 2:
    raise SystemExit("bench_accum.py: --accum must be >= 2 (bench.py measures the plain step)")
dev = torch.device("cuda", 0)
ops.set_mfma_precision(args.dtype)
os.environ["ADNM_AUTO_DDP"] = "0"
model = create_ADNMUNet(5, 20, 6, img_size=args.size)
recipe.fill_parameters(model)
model = model.to(dev).train()
K = args.accum
tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0).to(dev), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                 use_graph=True, accum_steps=K)
frames = recipe.radar_batch(args.batch, 25, args.size, name="bench").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
tr.prepare(x, tgt)
for _ in range(args.warmup * K):
    tr.step(x, tgt)
torch.cuda.synchronize()
windows = []
for _ in range(3):
    t0 = time.perf_counter()
    for _ in range(args.cycles * K):
        loss = tr.step(x, tgt)
    torch.cuda.synchronize()
    windows.append(1e3 * (time.perf_counter() - t0) / args.cycles)
loss = float(loss)
assert tr.micro_step == 0


def counted(n):
    """library launches of the next n eagerly launched micro-steps, one figure each, and the grad_accum* rows among them"""
    out = []
    for _ in range(n):
        lib.query("adnm_prof_enable", 1)
        tr.step(x, tgt, eager=True)
        torch.cuda.synchronize()
        lib.query("adnm_prof_enable", 0)
        buf = ctypes.create_string_buffer(1 << 20)
        lib.query("adnm_prof_collect", buf, len(buf))
        rows = [l.split("\t") for l in buf.value.decode().splitlines() if l.strip()]
        out.append((sum(int(r[1]) for r in rows), {r[0]: int(r[1]) for r in rows if r[0].startswith("grad_accum")}))
    return out


for _ in range(K):   # one eager cycle first: whatever an eager launch sets up once is not counted
    tr.step(x, tgt, eager=True)
torch.cuda.synchronize()
per = counted(K)
cycle = statistics.median(windows)
print(json.dumps({"metric": f"ADNM-UNet 5->20 {args.size}x{args.size} micro-batch {args.batch} x accum {K} {args.dtype} FlatTrainer graph replay",
                  "ms_per_cycle": round(cycle, 3), "ms_per_micro_step": round(cycle / K, 3),
                  "windows_ms_per_cycle": [round(w, 3) for w in windows], "windows_ms_per_micro_step": [round(w / K, 3) for w in windows],
                  "cycles_per_window": args.cycles, "optimizer_steps": tr._steps,
                  "launches_first_micro_step": per[0][0], "launches_micro_step": per[1][0] if K > 2 else None, "launches_final_step": per[-1][0],
                  "accum_launches": {"first": per[0][1], "middle": per[1][1] if K > 2 else None, "final": per[-1][1]}, "loss": loss}))
tr.close()
