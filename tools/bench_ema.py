#!/usr/bin/env python3
"""One record of what FlatTrainer(ema_decay=...) costs on bench.py's workload (ADNM-UNet 5 -> 20, recipe batch "bench", hipGraph replay),
measured in ONE session: two trainers live side by side in one process,
  plain   ema_decay=None    (the step as it was: the reference)
  ema     ema_decay=0.999   (adnm_ema_update behind every optimiser pass)
both prepared and warmed up, then timed in ALTERNATING windows (plain, ema, plain, ema, ...) of --steps steps each, so that drift of
the clock or of the shared host lands on both alike; reported: every window, the medians, their difference.  Then `ema_weights()`:
--windows times one enter + exit (swap, shadow rewrite, swap back, shadow rewrite) with a device synchronise on both sides.
bench.py measures the plain step and has no EMA switch.  --tail as in tools/bench_monitor.py: eager = one forward / backward graph and
the tail's launches from the host (bench.py's one-GPU configuration); graph = overlap=True, the tail captured and replayed.
f32 / bf16 only: two fp8 trainers would share one quantisation table.
The kernel durations (adnm_ema_update beside the AdamW pass) come from a kernel trace of this same program, e.g.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/bench_ema.py --windows 1 --steps 10 --out /dev/null
Run on the GPU box, under a time limit: timeout 600 python tools/bench_ema.py [--tail eager --batch 4 --size 128 --dtype bf16 --steps 40 --warmup 10]
Writes the result line to --out (default profiles/ema_bench.txt) and prints it."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import torch
from adnm_hip import ops, recipe
from adnm_hip.trainer import FlatTrainer
from models.ADNMUNet import create_ADNMUNet
from models.loss import enRainfallLoss

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16"])
ap.add_argument("--steps", type=int, default=40, help="timed steps per window")
ap.add_argument("--windows", type=int, default=5, help="windows per leg, alternating")
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--tail", default="eager", choices=["eager", "graph"], help="eager: one graph + host-launched tail (bench.py's); graph: staged, captured tail graph")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_ema.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
ops.set_mfma_precision(args.dtype)
os.environ["ADNM_AUTO_DDP"] = "0"
frames = recipe.radar_batch(args.batch, 25, args.size, name="bench").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()


def trainer(ema_decay):
    model = create_ADNMUNet(5, 20, 6, img_size=args.size)
    recipe.fill_parameters(model)
    model = model.to(dev).train()
    tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0).to(dev), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2,
                     max_norm=0.025, use_graph=True, overlap=args.tail == "graph", ema_decay=ema_decay)
    tr.prepare(x, tgt)
    assert (tr.tail is not None) == (args.tail == "graph")
    for _ in range(args.warmup):
        tr.step(x, tgt)
    torch.cuda.synchronize()
    return tr


def window(tr):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        tr.step(x, tgt)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.steps


legs = {"plain": trainer(None), "ema": trainer(0.999)}
try:
    ms = {k: [] for k in legs}
    for _ in range(args.windows):
        for k, tr in legs.items():
            ms[k].append(window(tr))
    tr = legs["ema"]
    info = tr.ema_info()
    assert info["updates"] == args.warmup + args.windows * args.steps, info
    ctx = []
    with tr.ema_weights():   # (the first one: code objects of the swap)
        pass
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with tr.ema_weights():
            pass
        torch.cuda.synchronize()
        ctx.append(1e3 * (time.perf_counter() - t0))
finally:
    for tr in legs.values():
        tr.close()

med = {k: statistics.median(v) for k, v in ms.items()}
line = json.dumps({"metric": f"ADNM-UNet 5->20 {args.size}x{args.size} batch {args.batch} {args.dtype} FlatTrainer graph replay, "
                             f"{'captured tail graph (overlap=True)' if args.tail == 'graph' else 'eager tail'}: ema_decay None / 0.999, alternating windows",
                   "tail": args.tail, "steps_per_window": args.steps, "parameters": int(legs["ema"].n),
                   "plain_ms_per_step": round(med["plain"], 4), "ema_ms_per_step": round(med["ema"], 4),
                   "plain_windows_ms": [round(w, 4) for w in ms["plain"]], "ema_windows_ms": [round(w, 4) for w in ms["ema"]],
                   "ema_minus_plain_us": round(1e3 * (med["ema"] - med["plain"]), 1),
                   "plain_spread_us": round(1e3 * (max(ms["plain"]) - min(ms["plain"])), 1),
                   "ema_weights_enter_exit_ms": round(statistics.median(ctx), 4), "ema_weights_windows_ms": [round(c, 4) for c in ctx],
                   "ema_info": info})
print(line)
with open(args.out, "w") as f:
    f.write(line + "\n")
