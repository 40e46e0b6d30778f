#!/usr/bin/env python3
"""One line for the record: N forecasts at config 2 (ADNM-UNet 5 -> 20, 128 x 128, batch 4, bf16) brought to the host as the bytes a
consumer keeps, timed two ways in ONE session on the same model, the legs interleaved (a b a b a b), median and spread of 3 windows:
  a   adnm_hip.forecast.Forecaster: one graph replay (forward + adnm_forecast_render), then .fields and .strip copied to pinned memory
  b   the route it replaces: a GraphedForward replay, .cpu() of the floats, then per frame on the host (seq * scale).astype(uint8)
      and a table lookup (numpy; matplotlib's norm + cmap per frame is slower still and is not what is timed), frames side by side
Both legs end with the same bytes on the host wherever numpy's cast is defined, which is checked: where pred * scale leaves [0, 256) (a model
on recipe parameters is not bounded) leg b holds whatever the host's float -> uint8 cast gives and leg a the documented clamp; the share of
such pixels is reported.  Bytes copied per pixel: a = 1 + 4 n / T, b = 4 (n of T frames selected).
The palette is tests/golden/forecast_palette_shanghai.json (data; the package ships no table).  bench.py is not involved.
Run on the GPU box, under a time limit: timeout 600 python tools/bench_forecast.py [--batches 16 --batch 4 --size 128 --dtype bf16 --warmup 3]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import numpy as np
import torch
from adnm_hip import ops, recipe
from adnm_hip.evaluator import GraphedForward
from adnm_hip.forecast import Forecaster, Palette
from models.ADNMUNet import create_ADNMUNet

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=16, help="N: forecasts per timed window")
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16", "fp8"])
ap.add_argument("--warmup", type=int, default=3, help="untimed forecasts per route before the windows")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_forecast.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
SCALE, START, STEP, GAP = 90.0, 1, 2, 10
pal = Palette.load(os.path.join(ROOT, "tests", "golden", "forecast_palette_shanghai.json"))
model = create_ADNMUNet(5, 20, 6, img_size=args.size)
recipe.fill_parameters(model)
model = model.to(dev).eval()
x = recipe.radar_batch(args.batch, 5, args.size, name="bench").to(dev)
if args.dtype == "fp8":
    with torch.no_grad():
        ops.fp8_calibrate(dev, lambda: model(x))
else:
    ops.set_mfma_precision(args.dtype)
fwd = GraphedForward(model)
fc = Forecaster(model, pal, pixel_scale=SCALE, frame_start=START, frame_step=STEP, gap=GAP)
host = {}


def route_a(n):
    for _ in range(n):
        res = fc(x)
        if not host:
            host["fields"], host["strip"] = torch.empty(res.fields.shape, dtype=torch.uint8).pin_memory(), torch.empty(res.strip.shape, dtype=torch.uint8).pin_memory()
        host["fields"].copy_(res.fields, non_blocking=True)
        host["strip"].copy_(res.strip, non_blocking=True)
        torch.cuda.current_stream().synchronize()        # the consumer reads the bytes now
    return host["fields"].numpy(), host["strip"].numpy()


EDGES, RGBA = np.asarray(pal.edges), pal.colours


def route_b(n):
    for _ in range(n):
        out = fwd(x).cpu().numpy()                        # the synchronising copy of B * T * H * W floats
        B, T = out.shape[:2]
        H, W = out.shape[-2:]
        fields = np.empty((B, T, H, W), dtype=np.uint8)
        sel = list(range(START, T, STEP))
        strip = np.full((B, H, len(sel) * W + (len(sel) - 1) * GAP, 4), 255, dtype=np.uint8)
        for b in range(B):
            seq = (out[b].squeeze() * SCALE).astype(np.uint8)
            fields[b] = seq
            for j, t in enumerate(sel):                   # frame by frame, as pic_results.py:143-170 goes
                idx = np.clip(np.searchsorted(EDGES, seq[t], side="right") - 1, 0, len(RGBA) - 1)
                strip[b, :, j * (W + GAP):j * (W + GAP) + W] = RGBA[idx]
    return fields, strip, out


def frames_of(strip, T, W):
    """(B, H, Ws, 4) -> (B, n, H, W, 4): the selected frames of a strip"""
    return np.stack([strip[:, :, j * (W + GAP):j * (W + GAP) + W] for j in range(len(range(START, T, STEP)))], axis=1)


try:
    route_a(args.warmup), route_b(args.warmup)
    torch.cuda.synchronize()
    windows, last = {"a": [], "b": []}, {}
    for _ in range(3):
        for key, route in (("a", route_a), ("b", route_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[key] = route(args.batches)
            torch.cuda.synchronize()
            windows[key].append(1e3 * (time.perf_counter() - t0))
    B, T, H, W = last["a"][0].shape
    n = len(range(START, T, STEP))
    prod = last["b"][2].reshape(B, T, H, W) * np.float32(SCALE)
    defined = (prod >= 0) & (prod < 256)                 # where (seq * scale).astype(np.uint8) means something
    same = bool(np.array_equal(last["a"][0][defined], last["b"][0][defined])
                and np.array_equal(frames_of(last["a"][1], T, W)[defined[:, START::STEP]], frames_of(last["b"][1], T, W)[defined[:, START::STEP]])
                and np.array_equal(last["a"][1][:, :, W:W + GAP], last["b"][1][:, :, W:W + GAP]))
finally:
    fwd.close()
    fc.close()
med = {k: statistics.median(w) for k, w in windows.items()}
print(json.dumps({"metric": f"{args.batches} forecasts to host bytes, ADNM-UNet 5->20 {args.size}x{args.size} batch {args.batch} {args.dtype}: "
                            "a = Forecaster + fields/strip to pinned memory, b = GraphedForward + .cpu() floats + numpy per frame",
                  "batches": args.batches, "a_ms": round(med["a"], 3), "b_ms": round(med["b"], 3),
                  "a_per_forecast_ms": round(med["a"] / args.batches, 3), "b_per_forecast_ms": round(med["b"] / args.batches, 3),
                  "a_windows_ms": [round(w, 3) for w in windows["a"]], "b_windows_ms": [round(w, 3) for w in windows["b"]],
                  "bytes_per_pixel": {"a": round(1 + 4 * n / T, 3), "b": 4}, "same_bytes_where_the_cast_is_defined": same,
                  "pixels_outside_the_uint8_range": round(1.0 - float(defined.mean()), 6),
                  "field_bytes_differing_in_all": int((last["a"][0] != last["b"][0]).sum())}))
