#!/usr/bin/env python3
"""One line for the record: a validation epoch of N batches at config 2 (ADNM-UNet 5 -> 20, 128 x 128, batch 4, bf16), timed two ways in
ONE session on the same model, the legs interleaved (a b a b a b), median and spread of 3 windows each:
  a   the route without adnm_hip.validate: GraphedForward, enRainfallLoss (value AND the unused gradient tensor) with .item() per batch,
      GpuEvaluator.evaluate per batch (a table and two workspaces allocated per call), done() at the end
  b   Validator: one graph replay per batch (forward, adnm_valid_accum, adnm_valid_ssim_accum), done() at the end
Also counted, on one batch of each route: the library entry points the HOST calls per batch (two kernel launches each) beside the
graph replay, and the host synchronisations.  bench.py measures the training step and is not involved.
Run on the GPU box, under a time limit: timeout 600 python tools/bench_validate.py [--batches 16 --batch 4 --size 128 --dtype bf16 --warmup 3]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import torch
from adnm_hip import lib, ops, recipe
from adnm_hip.evaluator import GpuEvaluator, GraphedForward
from adnm_hip.validate import Validator
from models.ADNMUNet import create_ADNMUNet
from models.loss import enRainfallLoss

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=16, help="N: batches per validation epoch (one timed window = one epoch)")
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16", "fp8"])
ap.add_argument("--warmup", type=int, default=3, help="untimed batches per route before the windows")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_validate.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
THR, SCALE = (20, 30, 35, 40), 255.0
model = create_ADNMUNet(5, 20, 6, img_size=args.size)
recipe.fill_parameters(model)
model = model.to(dev).eval()
crit = enRainfallLoss(0.57, 0.25, gamma=0.0)
frames = recipe.radar_batch(args.batch, 25, args.size, name="bench").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
if args.dtype == "fp8":
    with torch.no_grad():
        ops.fp8_calibrate(dev, lambda: model(x))
else:
    ops.set_mfma_precision(args.dtype)
fwd, val = GraphedForward(model), Validator(model, crit, 20, SCALE, THR)


def epoch_a(n):
    ev, loss_sum = GpuEvaluator(20, SCALE, THR), 0.0
    for _ in range(n):
        out = fwd(x)
        loss_sum += crit(out, tgt).item()
        ev.evaluate(tgt, out)
    res = ev.done()
    res["loss_sum"] = loss_sum
    return res


def epoch_b(n):
    for _ in range(n):
        val.step(x, tgt)
    return val.done(reset=True)


def entry_points(route):
    """library entry points the host calls for ONE batch of a route (the launches inside the replayed graph are not the host's)"""
    names, real = [], lib.call
    lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    try:
        route(1)
    finally:
        lib.call = real
    return names


try:
    epoch_a(args.warmup), epoch_b(args.warmup)
    calls = {"a": entry_points(epoch_a), "b": entry_points(epoch_b)}
    torch.cuda.synchronize()
    windows, last = {"a": [], "b": []}, {}
    for _ in range(3):
        for key, route in (("a", epoch_a), ("b", epoch_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[key] = route(args.batches)
            torch.cuda.synchronize()
            windows[key].append(1e3 * (time.perf_counter() - t0))
finally:
    fwd.close()
    val.close()
med = {k: statistics.median(w) for k, w in windows.items()}
spread_a = max(windows["a"]) - min(windows["a"])
print(json.dumps({"metric": f"validation epoch of {args.batches} batches, ADNM-UNet 5->20 {args.size}x{args.size} batch {args.batch} {args.dtype}: "
                            "a = GraphedForward + enRainfallLoss.item() + GpuEvaluator per batch, b = Validator",
                  "batches": args.batches,
                  "a_ms": round(med["a"], 3), "b_ms": round(med["b"], 3), "a_windows_ms": [round(w, 3) for w in windows["a"]],
                  "b_windows_ms": [round(w, 3) for w in windows["b"]], "a_spread_ms": round(spread_a, 3),
                  "b_minus_a_ms": round(med["b"] - med["a"], 3), "b_not_slower_beyond_spread": bool(med["b"] <= med["a"] + spread_a),
                  "per_batch": {"a": {"graph_replays": 1, "host_entry_points": calls["a"], "host_kernel_launches": 2 * len(calls["a"]), "host_syncs": 1},
                                "b": {"graph_replays": 1, "host_entry_points": calls["b"], "host_kernel_launches": 2 * len(calls["b"]), "host_syncs": 0}},
                  "loss_sum": {"a": last["a"]["loss_sum"], "b": last["b"]["loss_sum"]},
                  "RMSE": {"a": last["a"]["RMSE"], "b": last["b"]["RMSE"]}}))
