#!/usr/bin/env python3
"""What the D4 test-time-augmentation ensemble costs, for the record (profiles/ensemble_bench.txt): ADNM-UNet 5 -> 20, 128 x 128, T = 20,
bf16, four thresholds, M = 8, ONE session, one model.
  1. Validator.step at batch 1 with ensemble=True beside a plain Validator.step at batch 8 (the same forward: what the members and the score
     add) and beside a plain one at batch 1 (what the ensemble costs a user), the legs interleaved (a b c a b c ...), median and spread of 5
     windows of N calls each, a host clock around work that ends in a device synchronise.
  2. the HIP-event time of one call of adnm_d4_members (both directions), adnm_valid_ens_accum and adnm_ensemble_product on an all-zero
     stack, on a sparse radar-like stack and on uniform noise, beside adnm_valid_accum on the same target, median of 20 after a warm-up; and
     adnm_valid_ens_accum's time as a fraction of its (M + 1) * 4 bytes per pixel at 6.3 TB/s, the rate a float4 copy reaches on this part.
Run on the GPU box, under a time limit: timeout 600 python tools/bench_ensemble.py [--steps 8 --out profiles/ensemble_bench.txt]"""
import argparse, ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import torch
from adnm_hip import lib, ops, recipe
from adnm_hip.validate import Validator
from models.ADNMUNet import create_ADNMUNet
from models.loss import enRainfallLoss

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=8, help="N: calls per timed window")
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16"])
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_ensemble.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
THR, SCALE, T, S, M, HBM = (20, 30, 35, 40), 255.0, 20, args.size, 8, 6.3e12
model = create_ADNMUNet(5, T, 6, img_size=S)
recipe.fill_parameters(model)
model = model.to(dev).eval()
crit = enRainfallLoss(0.57, 0.25, gamma=0.0)
frames = recipe.radar_batch(M, 25, S, name="bench").to(dev)
x8, t8 = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
x1, t1 = x8[:1].contiguous(), t8[:1].contiguous()
ops.set_mfma_precision(args.dtype)
legs = {"ensemble B=1": (Validator(model, crit, T, SCALE, THR, ensemble=True), x1, t1), "plain B=8": (Validator(model, crit, T, SCALE, THR), x8, t8),
        "plain B=1": (Validator(model, crit, T, SCALE, THR), x1, t1)}


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


try:
    for val, x, tgt in legs.values():
        for _ in range(args.warmup):
            val.step(x, tgt)
    torch.cuda.synchronize()
    windows = {k: [] for k in legs}
    for _ in range(5):
        for key, (val, x, tgt) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                val.step(x, tgt)
            torch.cuda.synchronize()
            windows[key].append(1e3 * (time.perf_counter() - t0) / args.steps)
    results = {k: v[0].done(reset=True) for k, v in legs.items()}
    # the entry points on the same tensors, outside any graph
    n, stream, F, hw = len(THR), torch.cuda.current_stream().cuda_stream, T, S * S
    thr_c, codes = (ctypes.c_float * n)(*THR), (ctypes.c_int * M)(*range(M))
    gen = torch.Generator(device=dev).manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")

    def radar(k):
        """about 90 % exact zeros, smooth blobs reaching past every threshold"""
        f = torch.zeros(k, S, S, device=dev)
        for _ in range(2):
            cy, cx, s = (torch.rand(k, 1, 1, device=dev, generator=gen) * v for v in (S, S, 0.12 * S))
            f += torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * (s + 1.0) ** 2)) * 0.5
        return torch.where(f < torch.quantile(f.reshape(k, -1), 0.9, dim=1).view(k, 1, 1), torch.zeros_like(f), f)
    base = radar(F)
    stacks = {"all zero": (torch.zeros(F, S, S, device=dev), torch.zeros(M, F, S, S, device=dev)),
              "sparse radar-like": (base, torch.stack([torch.roll(base, m % 3, dims=2) * (1.0 - 0.03 * m) for m in range(M)])),
              "uniform noise": (torch.rand(F, S, S, device=dev, generator=gen), torch.rand(M, F, S, S, device=dev, generator=gen))}
    block = torch.zeros(lib.query("adnm_valid_block_bytes", T, n) // 8, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.query("adnm_valid_accum_ws_bytes", F, T, hw, n), dtype=torch.uint8, device=dev)
    table = torch.zeros(lib.query("adnm_valid_ens_block_bytes", T, n, M) // 8, dtype=torch.float64, device=dev)
    mean, prob, turned = torch.empty(F, S, S, device=dev), torch.empty(n, F, S, S, device=dev), torch.empty(M, F, S, S, device=dev)
    events, dry = {}, {}
    for name, (tg, mem) in stacks.items():
        calls = {"adnm_valid_accum (member 0)": lambda: lib.call("adnm_valid_accum", mem.data_ptr(), tg.data_ptr(), block.data_ptr(), None, thr_c, n, SCALE, 0.57, 0.25,
                                                                 0.0, ws.data_ptr(), ws.numel(), F, T, hw, stream),
                 "adnm_d4_members forward": lambda: ops.d4_members_into(tg, turned, codes, M, False),
                 "adnm_d4_members inverse": lambda: ops.d4_members_into(mem, turned, codes, M, True),
                 "adnm_valid_ens_accum": lambda: ops.ensemble_accum_into(mem, F * hw, T * hw, hw, tg, table, thr_c, n, SCALE, M, F, T, hw),
                 "adnm_ensemble_product": lambda: ops.ensemble_product_into(mem, F * hw, T * hw, hw, mean, prob, thr_c, n, SCALE, M, F, T, hw)}
        events[name] = {k: event_ms(fn) for k, fn in calls.items()}
        dry[name] = float(((tg * SCALE < 1.0) & (mem * SCALE < 1.0).all(dim=0)).float().mean())
finally:
    for val, _, _ in legs.values():
        val.close()
med = {k: statistics.median(w) for k, w in windows.items()}
spread = {k: max(w) - min(w) for k, w in windows.items()}
lines = [f"ADNM-UNet 5->{T} {S}x{S} {args.dtype}, M = {M}, thresholds {THR}; ms per Validator.step: median of 5 interleaved windows of {args.steps} calls (spread = max - min)"]
for k in legs:
    lines.append(f"  {k:14s} {med[k]:8.3f} ms  spread {spread[k]:.3f}   windows {[round(w, 3) for w in windows[k]]}")
lines.append(f"  ensemble B=1 - plain B=8 (the members, their undoing and the score): {med['ensemble B=1'] - med['plain B=8']:+.3f} ms; "
             f"ensemble B=1 / plain B=1 (what the ensemble costs): {med['ensemble B=1'] / med['plain B=1']:.2f} x")
traffic = (M + 1) * 4.0 * F * hw
lines.append(f"one call on the same tensors ({M} members of {F} frames of {S}x{S}; the score reads (M + 1) * 4 bytes per pixel = {traffic / 1e6:.2f} MB, "
             f"{1e6 * traffic / HBM:.1f} us at {HBM / 1e12:.1f} TB/s), HIP events, median (min .. max) of 20:")
for name, ev in events.items():
    lines.append(f"  {name} (dry pixels: {100 * dry[name]:.1f} %)")
    for k, (m, lo, hi) in ev.items():
        lines.append(f"    {k:28s} {1e3 * m:8.1f} us  ({1e3 * lo:.1f} .. {1e3 * hi:.1f})")
    lines.append(f"    adnm_valid_ens_accum runs at {100 * (traffic / HBM) / (1e-3 * ev['adnm_valid_ens_accum'][0]):.1f} % of its traffic at the HBM rate")
cheapest = min(events, key=lambda k: events[k]["adnm_valid_ens_accum"][0])
lines.append(f"  the cheapest adnm_valid_ens_accum input: {cheapest}" + ("" if cheapest == "all zero" else "  (NOT the all-zero stack: the ballot path is not doing its job)"))
e = results["ensemble B=1"]["ensemble"]
lines.append("checks: " + json.dumps({"members": e["members"], "pixels": int(e["pixels"]), "dry": int(e["dry"]),
                                      **{k: float(e[k]) for k in ("crps", "crps_fair", "mae_control", "crpss", "spread", "rmse_mean", "spread_skill")}}))
text = "\n".join(lines)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
