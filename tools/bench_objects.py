#!/usr/bin/env python3
"""What the object scores cost, for the record (profiles/objects_bench.txt): config 2 (ADNM-UNet 5 -> 20, 128 x 128, batch 4, T = 20,
bf16), four thresholds, ONE session, one model.
  1. Validator.step for two configurations, the legs interleaved (a b a b ...), median and spread of 5 windows of N steps each, a host
     clock around work that ends in a device synchronise:
       plain         Validator(...)                                   the parent's behaviour, the baseline
       objects       objects=True
  2. the HIP-event time of one adnm_valid_objects_accum call beside one adnm_valid_accum call on the same tensors, median of 20 after a
     warm-up, for four pairs of fields:
       zero          both fields all zero: staging the bits and the empty passes alone
       sparse        smooth blobs over about 90 % zeros, the forecast a blurred, shifted copy: what a radar field looks like
       noise41       independent noise with 41 % events at every threshold: around the 8-connected percolation point, the most tangled shapes
       serpentine    a one-pixel-wide path through the whole frame: ONE object, the worst case for propagation
     If the serpentine call takes more than about ten times the sparse one, the labelling is not converging as label equivalence should.
Run on the GPU box, under a time limit: timeout 600 python tools/bench_objects.py [--steps 16 --out profiles/objects_bench.txt]"""
import argparse, ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import torch
from adnm_hip import lib, ops, recipe
from adnm_hip.validate import Validator
from models.ADNMUNet import create_ADNMUNet
from models.loss import enRainfallLoss

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=16, help="N: Validator.step calls per timed window")
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16"])
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_bench.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_objects.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
THR, SCALE, T, S, B = (20, 30, 35, 40), 90.0, 20, args.size, args.batch
model = create_ADNMUNet(5, T, 6, img_size=S)
recipe.fill_parameters(model)
model = model.to(dev).eval()
crit = enRainfallLoss(0.57, 0.25, gamma=0.0)
frames = recipe.radar_batch(B, 25, S, name="bench").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
ops.set_mfma_precision(args.dtype)
legs = {"plain": Validator(model, crit, T, SCALE, THR), "objects": Validator(model, crit, T, SCALE, THR, objects=True)}


def window(val, n):
    for _ in range(n):
        val.step(x, tgt)


def event_ms(fn, n=20):
    for _ in range(3):
        fn()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def field_pairs():
    """-> {name: (target, forecast)}, fp32 (B * T, S, S) on the host"""
    g = torch.Generator(device="cpu").manual_seed(5)
    n = B * T
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    blobs = torch.zeros(n, S, S)
    for i in range(n):
        for _ in range(3):
            cy, cx, s, a = (torch.rand(1, generator=g).item() for _ in range(4))
            blobs[i] += (0.3 + 0.6 * a) * torch.exp(-((yy - cy * S) ** 2 + (xx - cx * S) ** 2) / (2 * (2.0 + 0.05 * S * s) ** 2))
    sparse_t = torch.where(blobs < torch.quantile(blobs.flatten()[::7], 0.9), torch.zeros(()), blobs)
    sparse_f = torch.roll(torch.nn.functional.avg_pool2d(sparse_t[:, None], 5, stride=1, padding=2)[:, 0], shifts=(2, 3), dims=(1, 2))
    sparse_f = torch.where(sparse_f < 0.02, torch.zeros(()), sparse_f)
    zero = torch.zeros(n, S, S)
    path = torch.zeros(S, S)
    path[0::2] = 1.0
    for i, y in enumerate(range(1, S - 1, 2)):
        path[y, S - 1 if i % 2 == 0 else 0] = 1.0
    path = path.expand(n, S, S).contiguous()
    return {"zero": (zero, zero.clone()), "sparse": (sparse_t, sparse_f),
            "noise41": ((torch.rand(n, S, S, generator=g) < 0.41).float(), (torch.rand(n, S, S, generator=g) < 0.41).float()),
            "serpentine": (path, torch.flip(path, dims=(1,)).contiguous())}


try:
    for val in legs.values():
        window(val, args.warmup)
    torch.cuda.synchronize()
    windows = {k: [] for k in legs}
    for _ in range(5):
        for key, val in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            window(val, args.steps)
            torch.cuda.synchronize()
            windows[key].append(1e3 * (time.perf_counter() - t0) / args.steps)
    results = {k: v.done(reset=True) for k, v in legs.items()}
    # the two entry points on the same tensors, outside any graph
    n, stream = len(THR), torch.cuda.current_stream().cuda_stream
    thr_c = (ctypes.c_float * n)(*THR)
    block = torch.zeros(lib.query("adnm_valid_block_bytes", T, n) // 8, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.query("adnm_valid_accum_ws_bytes", B * T, T, S * S, n), dtype=torch.uint8, device=dev)
    table = torch.zeros(lib.query("adnm_valid_objects_block_bytes", T, n) // 8, dtype=torch.float64, device=dev)
    nb = lib.query("adnm_valid_objects_accum_ws_bytes", B * T, T, S, S, n)
    ws_o = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    events, facts = {}, {}
    for name, (tg, pred) in field_pairs().items():
        tg, pred = tg.to(dev).contiguous(), pred.to(dev).contiguous()
        st = ops.object_stats(tg, pred, THR, SCALE)
        facts[name] = {"event_fraction_target_at_20": round(float(st[:, 0, 0, 1].sum()) / (B * T * S * S), 4),
                       "objects_per_frame_target_at_20": round(float(st[:, 0, 0, 0].sum()) / (B * T), 2),
                       "largest_object_target_at_20": int(st[:, 0, 0, 3].max())}
        events[name] = {
            "adnm_valid_accum": event_ms(lambda: lib.call("adnm_valid_accum", pred.data_ptr(), tg.data_ptr(), block.data_ptr(), None, thr_c, n, SCALE, 0.57, 0.25,
                                                          0.0, ws.data_ptr(), ws.numel(), B * T, T, S * S, stream)),
            "adnm_valid_objects_accum": event_ms(lambda: lib.call("adnm_valid_objects_accum", pred.data_ptr(), T * S * S, S * S, tg.data_ptr(), table.data_ptr(), thr_c,
                                                                  n, SCALE, 1, ws_o.data_ptr(), nb, B * T, T, S, S, stream))}
finally:
    for val in legs.values():
        val.close()
med = {k: statistics.median(w) for k, w in windows.items()}
spread = {k: max(w) - min(w) for k, w in windows.items()}
mb = 8.0 * B * T * S * S / 1e6
lines = [f"Validator.step, ADNM-UNet 5->{T} {S}x{S} batch {B} {args.dtype}, value_scale {SCALE:g}, thresholds {list(THR)}, ms per step: median of 5 interleaved windows of "
         f"{args.steps} steps (spread = max - min)"]
for k in legs:
    lines.append(f"  {k:12s} {med[k]:8.3f} ms  spread {spread[k]:.3f}  vs plain {med[k] - med['plain']:+.3f} ms   windows {[round(w, 3) for w in windows[k]]}")
lines.append(f"one call on the same tensors ({B * T} frames of {S}x{S}, {n} thresholds: {B * T * n} workgroups; forecast + target = {mb:.2f} MB; objects table "
             f"{table.numel() * 8} bytes, workspace {nb} bytes), HIP events, every launch of the entry point, median (min .. max) of 20:")
for name, ev in events.items():
    lines.append(f"  {name}: {json.dumps(facts[name])}")
    for k, (m, lo, hi) in ev.items():
        lines.append(f"    {k:28s} {1e3 * m:8.1f} us  ({1e3 * lo:.1f} .. {1e3 * hi:.1f})")
    lines.append(f"    objects / adnm_valid_accum = {ev['adnm_valid_objects_accum'][0] / ev['adnm_valid_accum'][0]:.2f}")
sp, se = events["sparse"]["adnm_valid_objects_accum"], events["serpentine"]["adnm_valid_objects_accum"]
lines.append(f"  convergence: serpentine {1e3 * se[0]:.1f} us against sparse {1e3 * sp[0]:.1f} us = {se[0] / sp[0]:.2f} x (about ten or more would mean the labels "
             "propagate step by step)")
ob = results["objects"]["objects"]
lines.append("checks: " + json.dumps({"plain_keys_unchanged": repr({k: results['objects'][k] for k in results['plain']}) == repr(results["plain"]),
                                      "target_area_equals_TP_plus_FN": all(ob[v]["target"]["area"] == int(results["objects"]["threshold_metrics"][v]["TP"]
                                                                                                       + results["objects"]["threshold_metrics"][v]["FN"]) for v in THR),
                                      "objects_at_20": {k: ob[20][k] for k in ("count_bias", "size_bias", "object_POD", "object_FAR", "object_CSI")},
                                      "target_at_20": {k: ob[20]["target"][k] for k in ("count", "per_frame", "mean_area", "weighted_area", "mean_largest")}}))
text = "\n".join(lines)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
