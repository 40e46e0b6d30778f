#!/usr/bin/env python3
"""What the intensity-scale skill score costs, for the record (profiles/iscale_bench.txt): config 2 (ADNM-UNet 5 -> 20, 128 x 128, batch 4,
T = 20, bf16, four thresholds), ONE session, one model.
  1. Validator.step plain, with intensity_scale=True, and with intensity_scale=True beside both baselines (persistence and advection, whose own
     pooled passes are timed in a leg of their own, so that the three intensity-scale passes are a difference of two legs), the legs
     interleaved (a b a b ...), median and spread of 5 windows of N calls each, a host clock around work that ends in a device synchronise.
  2. the HIP-event time of one adnm_valid_iscale_accum call on an all-zero pair, on a sparse radar-like pair and on 41 % noise, each beside
     adnm_valid_fss_accum at scales 1 5 17 33 and at scale 1 alone (the same event bits staged: the difference is the halo, the sliding sums
     and the products per pixel) and adnm_valid_accum on the same tensors, median of 20 after a warm-up.
Run on the GPU box, under a time limit: timeout 600 python tools/bench_iscale.py [--steps 16 --out profiles/iscale_bench.txt]"""
import argparse, ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import torch
from adnm_hip import lib, ops, recipe
from adnm_hip.validate import Validator
from models.ADNMUNet import create_ADNMUNet
from models.loss import enRainfallLoss

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=16, help="N: calls per timed window")
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16"])
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iscale_bench.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_iscale.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
THR, SCALE, T, S, B = (20, 30, 35, 40), 255.0, 20, args.size, args.batch
FSS = (1, 5, 17, 33)
model = create_ADNMUNet(5, T, 6, img_size=S)
recipe.fill_parameters(model)
model = model.to(dev).eval()
crit = enRainfallLoss(0.57, 0.25, gamma=0.0)
frames = recipe.radar_batch(B, 25, S, name="bench").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
ops.set_mfma_precision(args.dtype)
both = dict(persistence=True, advection=True)
legs = {"plain": Validator(model, crit, T, SCALE, THR), "iscale": Validator(model, crit, T, SCALE, THR, intensity_scale=True),
        "baselines": Validator(model, crit, T, SCALE, THR, **both), "iscale+baselines": Validator(model, crit, T, SCALE, THR, intensity_scale=True, **both)}


def window(leg, n):
    for _ in range(n):
        leg.step(x, tgt)


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
    for leg in legs.values():
        window(leg, args.warmup)
    torch.cuda.synchronize()
    windows = {k: [] for k in legs}
    for _ in range(5):
        for key, leg in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            window(leg, args.steps)
            torch.cuda.synchronize()
            windows[key].append(1e3 * (time.perf_counter() - t0) / args.steps)
    results = {k: v.done(reset=True) for k, v in legs.items()}
    # the entry points on the same tensors, outside any graph
    n, stream, F = len(THR), torch.cuda.current_stream().cuda_stream, B * T
    thr_c, tab, one = (ctypes.c_float * n)(*THR), ops.fss_table(FSS), ops.fss_table((1,))
    gen = torch.Generator(device=dev).manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")

    def radar():
        """about 90 % exact zeros, smooth blobs reaching past every threshold"""
        f = torch.zeros(F, S, S, device=dev)
        for _ in range(2):
            cy, cx, s = (torch.rand(F, 1, 1, device=dev, generator=gen) * v for v in (S, S, 0.12 * S))
            f += torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * (s + 1.0) ** 2)) * 0.5
        return torch.where(f < torch.quantile(f.reshape(F, -1), 0.9, dim=1).view(F, 1, 1), torch.zeros_like(f), f)

    def noise():
        return torch.where(torch.rand(F, S, S, device=dev, generator=gen) < 0.41, torch.full((F, S, S), 0.5, device=dev), torch.zeros(F, S, S, device=dev))
    pairs = {"all zero": (torch.zeros(F, S, S, device=dev), torch.zeros(F, S, S, device=dev)), "sparse radar-like": (radar(), torch.roll(radar(), 2, dims=2)),
             "41 % noise": (noise(), noise())}
    block = torch.zeros(lib.query("adnm_valid_block_bytes", T, n) // 8, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.query("adnm_valid_accum_ws_bytes", F, T, S * S, n), dtype=torch.uint8, device=dev)
    t_fss = torch.zeros(lib.query("adnm_valid_fss_block_bytes", T, n, len(FSS)) // 8, dtype=torch.float64, device=dev)
    ws_f = torch.empty(lib.query("adnm_valid_fss_accum_ws_bytes", F, T, S, S, n, tab, len(FSS)), dtype=torch.uint8, device=dev)
    t_is = torch.zeros(lib.query("adnm_valid_iscale_block_bytes", T, n, S, S) // 8, dtype=torch.float64, device=dev)
    ws_i = torch.empty(lib.query("adnm_valid_iscale_accum_ws_bytes", F, T, S, S, n), dtype=torch.uint8, device=dev)
    events, events_frac = {}, {}
    for name, (tg, pr) in pairs.items():
        def fss(table, count, pr=pr, tg=tg):
            return lambda: lib.call("adnm_valid_fss_accum", pr.data_ptr(), T * S * S, S * S, tg.data_ptr(), t_fss.data_ptr(), thr_c, n, SCALE, table, count,
                                    ws_f.data_ptr(), ws_f.numel(), F, T, S, S, stream)
        calls = {"adnm_valid_accum": lambda: lib.call("adnm_valid_accum", pr.data_ptr(), tg.data_ptr(), block.data_ptr(), None, thr_c, n, SCALE, 0.57, 0.25, 0.0,
                                                      ws.data_ptr(), ws.numel(), F, T, S * S, stream),
                 "adnm_valid_fss_accum, 4 scales": fss(tab, len(FSS)), "adnm_valid_fss_accum, scale 1": fss(one, 1),
                 "adnm_valid_iscale_accum": lambda: lib.call("adnm_valid_iscale_accum", pr.data_ptr(), T * S * S, S * S, tg.data_ptr(), t_is.data_ptr(), thr_c, n, SCALE,
                                                             ws_i.data_ptr(), ws_i.numel(), F, T, S, S, stream)}
        events[name] = {k: event_ms(fn) for k, fn in calls.items()}
        events_frac[name] = float((pr * SCALE >= THR[0]).float().mean())
finally:
    for leg in legs.values():
        leg.close()
med = {k: statistics.median(w) for k, w in windows.items()}
spread = {k: max(w) - min(w) for k, w in windows.items()}
mb = 8.0 * B * T * S * S / 1e6
lines = [f"Validator.step, ADNM-UNet 5->{T} {S}x{S} batch {B} {args.dtype}, ms per step: median of 5 interleaved windows of {args.steps} steps (spread = max - min)"]
for k, base in (("plain", "plain"), ("iscale", "plain"), ("baselines", "plain"), ("iscale+baselines", "baselines")):
    lines.append(f"  {k:18s} {med[k]:8.3f} ms  spread {spread[k]:.3f}  vs {base} {med[k] - med[base]:+.3f} ms   windows {[round(w, 3) for w in windows[k]]}")
lines.append(f"one call on the same tensors ({B * T} frames of {S}x{S}; forecast + target = {mb:.2f} MB; thresholds {THR}), HIP events, every launch of the entry point, "
             "median (min .. max) of 20:")
for name, ev in events.items():
    lines.append(f"  {name} (forecast events at {THR[0]}: {100 * events_frac[name]:.1f} % of the pixels)")
    for k, (m, lo, hi) in ev.items():
        lines.append(f"    {k:32s} {1e3 * m:8.1f} us  ({1e3 * lo:.1f} .. {1e3 * hi:.1f})")
    lines.append(f"    iscale / fss (4 scales) = {ev['adnm_valid_iscale_accum'][0] / ev['adnm_valid_fss_accum, 4 scales'][0]:.2f}   "
                 f"iscale / fss (scale 1) = {ev['adnm_valid_iscale_accum'][0] / ev['adnm_valid_fss_accum, scale 1'][0]:.2f}")
e = results["iscale+baselines"]
lines.append("checks: " + json.dumps({
    "plain_keys_unchanged": repr({k: results["iscale"][k] for k in results["plain"]}) == repr(results["plain"]),
    "scale_px": e["intensity_scale"]["scale_px"].tolist(),
    "skill20": {name: [round(float(v), 4) for v in ent["intensity_scale"][20]["skill"]] for name, ent in (("forecast", e), ("persistence", e["persistence"]),
                                                                                                          ("advection", e["advection"]))}}))
text = "\n".join(lines)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
