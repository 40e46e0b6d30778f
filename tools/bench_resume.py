#!/usr/bin/env python3
"""Three lines for the record: what saving the training state costs the step on bench.py's workload (config 2: ADNM-UNet 5 -> 20,
128 x 128, B = 4, bf16, recipe batch "bench"), FlatTrainer hipGraph replay —
  plain      no saving;
  snapshot   FlatTrainer.snapshot() every --every steps (device-to-device copies behind the step; the snapshot is turned into the host
             dict, TrainerSnapshot.state_dict(), by a second thread on a side stream, as a checkpoint writer would);
  sync       FlatTrainer.state_dict() every --every steps (the training stream waits for the device -> host copies and the packing).
ms per step over all timed steps, the saving ones included (median of 3 windows).  bench.py measures the plain step only.
Run on the GPU box: python tools/bench_resume.py [--every 50 --steps 100 --batch 4 --size 128 --dtype bf16 --warmup 5]"""
import argparse, json, os, statistics, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import torch
from adnm_hip import ops, recipe
from adnm_hip.trainer import FlatTrainer
from models.ADNMUNet import create_ADNMUNet
from models.loss import enRainfallLoss

ap = argparse.ArgumentParser()
ap.add_argument("--every", type=int, default=50, help="steps between two saves")
ap.add_argument("--steps", type=int, default=100, help="timed steps per window (3 windows per case)")
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16", "fp8"])
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_resume.py: no GPU (a timing without one would mean nothing)")
if args.every < 1 or args.steps < args.every:
    raise SystemExit("bench_resume.py: --steps must cover at least one save (--steps >= --every >= 1)")
dev = torch.device("cuda", 0)
ops.set_mfma_precision(args.dtype)
os.environ["ADNM_AUTO_DDP"] = "0"
model = create_ADNMUNet(5, 20, 6, img_size=args.size)
recipe.fill_parameters(model)
model = model.to(dev).train()
tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0).to(dev), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                 use_graph=True)
frames = recipe.radar_batch(args.batch, 25, args.size, name="bench").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
tr.prepare(x, tgt)
for _ in range(args.warmup):
    tr.step(x, tgt)
torch.cuda.synchronize()


def window(case):
    writers = []
    t0 = time.perf_counter()
    for i in range(1, args.steps + 1):
        tr.step(x, tgt)
        if i % args.every == 0:
            if case == "snapshot":
                w = threading.Thread(target=tr.snapshot().state_dict)
                w.start()
                writers.append(w)
            elif case == "sync":
                tr.state_dict()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for w in writers:   # (the writers' host work is not the step's: joined outside the timed span)
        w.join()
    return 1e3 * dt / args.steps


for case in ("plain", "snapshot", "sync"):
    window(case)   # one untimed window: allocations of the case's first save
    ws = [window(case) for _ in range(3)]
    print(json.dumps({"metric": f"ADNM-UNet 5->20 {args.size}x{args.size} B={args.batch} {args.dtype} FlatTrainer graph replay, state saved: {case}",
                      "every": None if case == "plain" else args.every, "steps_per_window": args.steps,
                      "ms_per_step": round(statistics.median(ws), 3), "windows_ms_per_step": [round(w, 3) for w in ws]}))
tr.close()
