#!/usr/bin/env python3
"""What the advection baseline costs, for the record (profiles/advect_bench.txt): config 2 (ADNM-UNet 5 -> 20, 128 x 128, batch 4, T = 20,
bf16), ONE session, one model.
  1. Validator.step for three configurations, the legs interleaved (a b c a b c ...), median and spread of 5 windows of N steps each,
     a host clock around work that ends in a device synchronise:
       plain         Validator(...)                                                   the baseline
       pers          persistence=True, fss=(1, 5, 17, 33), pools=(4, 16)               the yardstick the advection is held against
       pers+adv      the same plus advection=True                                     (+ trec_cost, trec_pick, advect, one pooled and one FSS pass)
  2. the HIP-event time of one adnm_trec_motion call (both launches; three block / radius pairs) and one adnm_advect call on the model's
     input, median of 20 after a warm-up, and each of the three launches (trec_cost, trec_pick, advect) alone from the library's own
     per-kernel events.
Run on the GPU box, under a time limit: timeout 600 python tools/bench_advect.py [--steps 16 --out profiles/advect_bench.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "advect_bench.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_advect.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
THR, SCALE, T, S, B = (20, 30, 35, 40), 255.0, 20, args.size, args.batch
FSS, POOLS = (1, 5, 17, 33), (4, 16)
model = create_ADNMUNet(5, T, 6, img_size=S)
recipe.fill_parameters(model)
model = model.to(dev).eval()
crit = enRainfallLoss(0.57, 0.25, gamma=0.0)
frames = recipe.radar_batch(B, 25, S, name="bench").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
ops.set_mfma_precision(args.dtype)
legs = {"plain": Validator(model, crit, T, SCALE, THR),
        "pers": Validator(model, crit, T, SCALE, THR, persistence=True, fss=FSS, pools=POOLS),
        "pers+adv": Validator(model, crit, T, SCALE, THR, persistence=True, fss=FSS, pools=POOLS, advection=True)}


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
    # the new launches on the model's input, outside any graph
    block, radius, echo = legs["pers+adv"].advection
    xin = x.reshape(B, 5, S, S)
    prev, last, stride, stream = xin.data_ptr() + 4 * 3 * S * S, xin.data_ptr() + 4 * 4 * S * S, 5 * S * S, torch.cuda.current_stream().cuda_stream
    nb = -(-S // block)
    motion = torch.zeros((B, nb, nb, 2), dtype=torch.int32, device=dev)
    out = torch.empty((B, T, S, S), dtype=torch.float32, device=dev)

    def motion_call(bl, r):
        w = torch.empty(lib.query("adnm_trec_ws_bytes", B, S, S, bl, r), dtype=torch.uint8, device=dev)
        m = torch.zeros((B, -(-S // bl), -(-S // bl), 2), dtype=torch.int32, device=dev)
        return lambda: lib.call("adnm_trec_motion", prev, last, stride, m.data_ptr(), None, SCALE, bl, r, echo, w.data_ptr(), w.numel(), B, S, S, stream)
    calls = {
        f"adnm_trec_motion (trec_cost + trec_pick), block {block} radius {radius}": motion_call(block, radius),
        "adnm_trec_motion, block 32 radius 8": motion_call(32, 8),
        "adnm_trec_motion, block 8 radius 2": motion_call(8, 2),
        f"adnm_advect, block {block}, T {T}": lambda: lib.call("adnm_advect", last, stride, motion.data_ptr(), out.data_ptr(), block, B, T, S, S, stream)}
    motion_call(block, radius)()
    events = {k: event_ms(fn) for k, fn in calls.items()}
    # each of the three launches alone: the library's own per-kernel events (include/adnm_hip.h: adnm_prof_*), 20 calls
    lib.query("adnm_prof_enable", 1)
    for _ in range(20):
        calls[f"adnm_trec_motion (trec_cost + trec_pick), block {block} radius {radius}"]()
        calls[f"adnm_advect, block {block}, T {T}"]()
    torch.cuda.synchronize()
    lib.query("adnm_prof_enable", 0)
    buf = ctypes.create_string_buffer(1 << 16)
    lib.query("adnm_prof_collect", buf, len(buf))
    kernels = {r[0].split("@")[0]: (int(r[1]), float(r[2])) for r in (l.split("\t") for l in buf.value.decode().splitlines() if l.strip())}
finally:
    for val in legs.values():
        val.close()
med = {k: statistics.median(w) for k, w in windows.items()}
spread = {k: max(w) - min(w) for k, w in windows.items()}
lines = [f"Validator.step, ADNM-UNet 5->{T} {S}x{S} batch {B} {args.dtype}, ms per step: median of 5 interleaved windows of {args.steps} steps (spread = max - min)"]
for k in legs:
    lines.append(f"  {k:12s} {med[k]:8.3f} ms  spread {spread[k]:.3f}  vs plain {med[k] - med['plain']:+.3f} ms   windows {[round(w, 3) for w in windows[k]]}")
lines.append(f"  pers+adv over pers {med['pers+adv'] - med['pers']:+.3f} ms; pers over plain {med['pers'] - med['plain']:+.3f} ms")
lines.append(f"one call on the model's input ({B} samples of {S}x{S}; advect writes {4.0 * B * T * S * S / 1e6:.2f} MB), HIP events, median (min .. max) of 20:")
for k, (m, lo, hi) in events.items():
    lines.append(f"  {k:70s} {1e3 * m:8.1f} us  ({1e3 * lo:.1f} .. {1e3 * hi:.1f})")
lines.append(f"each launch alone, block {block} radius {radius}, mean of the library's per-kernel events:")
for k in (k for k in ("trec_cost", "trec_pick", "advect") if k in kernels):
    lines.append(f"  {k:70s} {1e3 * kernels[k][1] / kernels[k][0]:8.1f} us  ({kernels[k][0]} launches)")
adv, pers = results["pers+adv"]["advection"], results["pers+adv"]["persistence"]
lines.append("checks: " + json.dumps({"former_keys_unchanged": repr({k: results['pers+adv'][k] for k in results['pers']}) == repr(results["pers"]),
                                      "advection_CSI": {str(t): adv["threshold_metrics"][t]["CSI"] for t in THR},
                                      "persistence_CSI": {str(t): pers["threshold_metrics"][t]["CSI"] for t in THR}}))
text = "\n".join(lines)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
