#!/usr/bin/env python3
"""One line for the record: the long-interval (LAPS) recipe, create_ADNMUNet(5, 3, 60), FlatTrainer hipGraph replay — ms / step and the
library's launches per step (counted by adnm_prof_* over one eagerly launched step).  bench.py measures the flagship 5 -> 20 recipe and has
no frame_interval switch.  Run on the GPU box: python tools/bench_laps.py [--size 128 --batch 4 --dtype bf16 --steps 60 --warmup 10]"""
import argparse, ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import torch
from adnm_hip import ops, lib, recipe
from adnm_hip.trainer import FlatTrainer
from models.ADNMUNet import create_ADNMUNet
from models.loss import enRainfallLoss

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16"])
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_laps.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
ops.set_mfma_precision(args.dtype)
os.environ["ADNM_AUTO_DDP"] = "0"
model = create_ADNMUNet(5, 3, 60, img_size=args.size)
recipe.fill_parameters(model)
model = model.to(dev).train()
tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0).to(dev), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                 use_graph=True)
frames = recipe.radar_batch(args.batch, 8, args.size, name="bench_laps").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
tr.prepare(x, tgt)
for _ in range(args.warmup):
    tr.step(x, tgt)
torch.cuda.synchronize()
windows, k = [], max(1, args.steps // 3)
for _ in range(3):
    t0 = time.perf_counter()
    for _ in range(k):
        loss = tr.step(x, tgt)
    torch.cuda.synchronize()
    windows.append(1e3 * (time.perf_counter() - t0) / k)
tr.step(x, tgt, eager=True)
torch.cuda.synchronize()
lib.query("adnm_prof_enable", 1)
tr.step(x, tgt, eager=True)
torch.cuda.synchronize()
lib.query("adnm_prof_enable", 0)
buf = ctypes.create_string_buffer(1 << 20)
lib.query("adnm_prof_collect", buf, len(buf))
rows = [l.split("\t") for l in buf.value.decode().splitlines() if l.strip()]
launches = sum(int(r[1]) for r in rows)
norm = {r[0].split("@")[0]: 0 for r in rows if r[0].startswith(("groupnorm", "instnorm"))}
for r in rows:
    if r[0].split("@")[0] in norm:
        norm[r[0].split("@")[0]] += int(r[1])
print(json.dumps({"metric": f"LAPS 5->3 {args.size}x{args.size} B={args.batch} {args.dtype} FlatTrainer graph replay", "ms_per_step": round(statistics.median(windows), 3),
                  "windows_ms": [round(w, 3) for w in windows], "launches_per_step": launches, "norm_launches": norm, "loss": float(loss)}))
tr.close()
