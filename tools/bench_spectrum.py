#!/usr/bin/env python3
"""What the power spectra cost, for the record (profiles/spectrum_bench.txt): config 2 (ADNM-UNet 5 -> 20, 128 x 128, batch 4, T = 20,
bf16), ONE session, one model.
  1. Validator.step for two configurations, the legs interleaved (a b a b ...), median and spread of 5 windows of N steps each, a host
     clock around work that ends in a device synchronise:
       plain         Validator(...)                                   the parent's behaviour, the baseline
       spectrum      spectrum=True
  2. the HIP-event time of one adnm_valid_spectrum_accum call (the contiguous forecast; the held input frame with frame stride 0) beside
     one adnm_valid_accum call on the same tensors (both read the forecast and the target once: 8 bytes per pixel), median of 20 after a
     warm-up.
Run on the GPU box, under a time limit: timeout 600 python tools/bench_spectrum.py [--steps 16 --out profiles/spectrum_bench.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_bench.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_spectrum.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
THR, SCALE, T, S, B = (20, 30, 35, 40), 255.0, 20, args.size, args.batch
model = create_ADNMUNet(5, T, 6, img_size=S)
recipe.fill_parameters(model)
model = model.to(dev).eval()
crit = enRainfallLoss(0.57, 0.25, gamma=0.0)
frames = recipe.radar_batch(B, 25, S, name="bench").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
ops.set_mfma_precision(args.dtype)
legs = {"plain": Validator(model, crit, T, SCALE, THR), "spectrum": Validator(model, crit, T, SCALE, THR, spectrum=True)}


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
    pred = legs["plain"].step(x, tgt).reshape(B, T, S, S).clone()
    tg = tgt.reshape(B, T, S, S).contiguous()
    n, stream = len(THR), torch.cuda.current_stream().cuda_stream
    thr_c = (ctypes.c_float * n)(*THR)
    block = torch.zeros(lib.query("adnm_valid_block_bytes", T, n) // 8, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.query("adnm_valid_accum_ws_bytes", B * T, T, S * S, n), dtype=torch.uint8, device=dev)
    table = torch.zeros(lib.query("adnm_valid_spectrum_block_bytes", T, S, S) // 8, dtype=torch.float64, device=dev)
    ws_s = torch.empty(lib.query("adnm_valid_spectrum_accum_ws_bytes", B * T, T, S, S), dtype=torch.uint8, device=dev)
    xin = x.reshape(B, 5, S, S)

    def spectrum_call(src, ss, fs):
        return lambda: lib.call("adnm_valid_spectrum_accum", src, ss, fs, tg.data_ptr(), table.data_ptr(), SCALE, ws_s.data_ptr(), ws_s.numel(), B * T, T, S, S,
                                stream)
    calls = {
        "adnm_valid_accum": lambda: lib.call("adnm_valid_accum", pred.data_ptr(), tg.data_ptr(), block.data_ptr(), None, thr_c, n, SCALE, 0.57, 0.25, 0.0,
                                             ws.data_ptr(), ws.numel(), B * T, T, S * S, stream),
        "adnm_valid_spectrum_accum": spectrum_call(pred.data_ptr(), T * S * S, S * S),
        "adnm_valid_spectrum_accum, held input frame": spectrum_call(xin.data_ptr() + 4 * 4 * S * S, 5 * S * S, 0)}
    events = {k: event_ms(fn) for k, fn in calls.items()}
finally:
    for val in legs.values():
        val.close()
med = {k: statistics.median(w) for k, w in windows.items()}
spread = {k: max(w) - min(w) for k, w in windows.items()}
mb = 8.0 * B * T * S * S / 1e6
lines = [f"Validator.step, ADNM-UNet 5->{T} {S}x{S} batch {B} {args.dtype}, ms per step: median of 5 interleaved windows of {args.steps} steps (spread = max - min)"]
for k in legs:
    lines.append(f"  {k:12s} {med[k]:8.3f} ms  spread {spread[k]:.3f}  vs plain {med[k] - med['plain']:+.3f} ms   windows {[round(w, 3) for w in windows[k]]}")
lines.append(f"one call on the same tensors ({B * T} frames of {S}x{S}; forecast + target = {mb:.2f} MB; spectrum workspace {ws_s.numel() / 1e6:.2f} MB), HIP events, "
             "every launch of the entry point, median (min .. max) of 20:")
for k, (m, lo, hi) in events.items():
    lines.append(f"  {k:45s} {1e3 * m:8.1f} us  ({1e3 * lo:.1f} .. {1e3 * hi:.1f})")
ratio = events["adnm_valid_spectrum_accum"][0] / events["adnm_valid_accum"][0]
lines.append(f"  spectrum / adnm_valid_accum = {ratio:.2f}")
sp = results["spectrum"]["spectrum"]
lines.append("checks: " + json.dumps({"plain_keys_unchanged": repr({k: results['spectrum'][k] for k in results['plain']}) == repr(results["plain"]),
                                      "ratio_at_wavelengths_px": {f"{sp['wavelength_px'][r]:.1f}": float(sp["ratio"][r]) for r in (1, 4, 16, 63) if r < len(sp["ratio"])},
                                      "coherence_at_wavelengths_px": {f"{sp['wavelength_px'][r]:.1f}": float(sp["coherence"][r]) for r in (1, 4, 16, 63) if r < len(sp["ratio"])},
                                      "effective_resolution_px": sp["effective_resolution_px"]}))
text = "\n".join(lines)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
