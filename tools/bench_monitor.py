#!/usr/bin/env python3
"""One line for the record: what FlatTrainer(monitor=True) costs on bench.py's workload (ADNM-UNet 5 -> 20, recipe batch "bench", hipGraph
replay), timed three ways in ONE session, a fresh model and trainer per leg, median of 3 windows of --steps steps each:
  off     monitor=False                                                  (the unmonitored step: the reference of the other two)
  on      monitor=True                                                   (guard + statistics on the device, stats() once per window)
  item    monitor=False, grad_norm().item() and loss.item() after every step   (what train.py:141-145 does)
and `off` once more at the end, as a check on drift within the session.  bench.py measures the plain step and has no monitor switch.
--tail says WHICH optimiser tail is timed, and the result line names it:
  eager   (default) one forward / backward graph, then the tail's launches from the host — bench.py's one-GPU configuration; the
          monitor adds its launches to that eager sequence;
  graph   overlap=True: the backward cut into stage graphs and the tail (guard, table update, AdamW) captured and replayed as the tail
          graph, the form every multi-GPU step takes — here on one GPU, without collectives.
Run on the GPU box, under a time limit: timeout 600 python tools/bench_monitor.py [--tail eager --batch 4 --size 128 --dtype bf16 --steps 40 --warmup 10]"""
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
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16", "fp8"])
ap.add_argument("--steps", type=int, default=40, help="timed steps per window (3 windows per leg)")
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--tail", default="eager", choices=["eager", "graph"], help="eager: one graph + host-launched tail (bench.py's); graph: staged, captured tail graph")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_monitor.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
ops.set_mfma_precision(args.dtype)
os.environ["ADNM_AUTO_DDP"] = "0"
frames = recipe.radar_batch(args.batch, 25, args.size, name="bench").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()


def leg(monitor, item):
    ops.QUANT.reset()
    model = create_ADNMUNet(5, 20, 6, img_size=args.size)
    recipe.fill_parameters(model)
    model = model.to(dev).train()
    tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0).to(dev), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2,
                     max_norm=0.025, use_graph=True, monitor=monitor, overlap=args.tail == "graph")
    try:
        tr.prepare(x, tgt)
        assert (tr.tail is not None) == (args.tail == "graph")
        for _ in range(args.warmup):
            tr.step(x, tgt)
        torch.cuda.synchronize()
        windows, seen = [], None
        for _ in range(3):
            norm_sum = loss_sum = 0.0
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = tr.step(x, tgt)
                if item:
                    norm_sum += tr.grad_norm().item()
                    loss_sum += loss.item()
            if monitor:
                st = tr.stats(reset=True)   # the epoch's one synchronising read, inside the window
                norm_sum, loss_sum = st["norm_sum"], st["loss_sum"]
                assert st["steps"] == args.steps and st["skipped"] == 0, st
            torch.cuda.synchronize()
            windows.append(1e3 * (time.perf_counter() - t0) / args.steps)
            seen = (norm_sum, loss_sum)
        return {"ms_per_step": round(statistics.median(windows), 4), "windows_ms": [round(w, 4) for w in windows],
                "last_window_norm_sum": seen[0], "last_window_loss_sum": seen[1]}
    finally:
        tr.close()


res = {"off": leg(False, False), "on": leg(True, False), "item": leg(False, True), "off_again": leg(False, False)}
base = res["off"]["ms_per_step"]
print(json.dumps({"metric": f"ADNM-UNet 5->20 {args.size}x{args.size} batch {args.batch} {args.dtype} FlatTrainer graph replay, {'captured tail graph (overlap=True)' if args.tail == 'graph' else 'eager tail'}: monitor off / on / per-step .item()",
                  "tail": args.tail,
                  "steps_per_window": args.steps, "legs": res,
                  "on_minus_off_us": round(1e3 * (res["on"]["ms_per_step"] - base), 1),
                  "item_minus_off_us": round(1e3 * (res["item"]["ms_per_step"] - base), 1),
                  "off_again_minus_off_us": round(1e3 * (res["off_again"]["ms_per_step"] - base), 1)}))
