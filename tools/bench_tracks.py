#!/usr/bin/env python3
"""What the track scores cost, for the record (profiles/tracks_bench.txt): config 2 (ADNM-UNet 5 -> 20, 128 x 128, batch 4, T = 20,
bf16), four thresholds, ONE session, one model.
  1. Validator.step for two configurations, the legs interleaved (a b a b ...), median and spread of 5 windows of N steps each, a host
     clock around work that ends in a device synchronise:
       plain         Validator(...)                                   the parent's behaviour, the baseline
       tracks        tracks=True
  2. the HIP-event time of one adnm_valid_tracks_accum call beside one adnm_valid_objects_accum and one adnm_valid_accum call on the same
     tensors, median of 20 after a warm-up, for three pairs of fields:
       zero          both fields all zero: staging the bits, writing the words and the empty passes alone
       sparse        smooth blobs over about 90 % zeros that drift 1 px per frame, the forecast a blurred, shifted copy: what a radar field looks like
       noise08       independent noise with 8 % events: just under the 26-neighbour site-percolation point, many tortuous tracks
     The objects pass labels the same voxels frame by frame, so tracks / objects is the cost of writing the words to memory, of the merge in
     time and of the two passes over the records.
Run on the GPU box, under a time limit: timeout 600 python tools/bench_tracks.py [--steps 16 --out profiles/tracks_bench.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracks_bench.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_tracks.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
THR, SCALE, T, S, B = (20, 30, 35, 40), 90.0, 20, args.size, args.batch
model = create_ADNMUNet(5, T, 6, img_size=S)
recipe.fill_parameters(model)
model = model.to(dev).eval()
crit = enRainfallLoss(0.57, 0.25, gamma=0.0)
frames = recipe.radar_batch(B, 25, S, name="bench").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
ops.set_mfma_precision(args.dtype)
legs = {"plain": Validator(model, crit, T, SCALE, THR), "tracks": Validator(model, crit, T, SCALE, THR, tracks=True)}


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
    """-> {name: (target, forecast)}, fp32 (B, T, S, S) on the host"""
    g = torch.Generator(device="cpu").manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    blobs = torch.zeros(B, T, S, S)
    for b in range(B):
        for _ in range(3):
            cy, cx, s, a, vy, vx = (torch.rand(1, generator=g).item() for _ in range(6))
            for t in range(T):
                oy, ox = cy * S + (2 * vy - 1) * t, cx * S + (2 * vx - 1) * t
                blobs[b, t] += (0.3 + 0.6 * a) * torch.exp(-((yy - oy) ** 2 + (xx - ox) ** 2) / (2 * (2.0 + 0.05 * S * s) ** 2))
    sparse_t = torch.where(blobs < torch.quantile(blobs.flatten()[::7], 0.9), torch.zeros(()), blobs)
    sparse_f = torch.roll(torch.nn.functional.avg_pool2d(sparse_t, 5, stride=1, padding=2), shifts=(2, 3), dims=(2, 3))
    sparse_f = torch.where(sparse_f < 0.02, torch.zeros(()), sparse_f)
    zero = torch.zeros(B, T, S, S)
    return {"zero": (zero, zero.clone()), "sparse": (sparse_t, sparse_f),
            "noise08": ((torch.rand(B, T, S, S, generator=g) < 0.08).float(), (torch.rand(B, T, S, S, generator=g) < 0.08).float())}


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
    # the three entry points on the same tensors, outside any graph
    n, stream = len(THR), torch.cuda.current_stream().cuda_stream
    thr_c = (ctypes.c_float * n)(*THR)
    block = torch.zeros(lib.query("adnm_valid_block_bytes", T, n) // 8, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.query("adnm_valid_accum_ws_bytes", B * T, T, S * S, n), dtype=torch.uint8, device=dev)
    table_o = torch.zeros(lib.query("adnm_valid_objects_block_bytes", T, n) // 8, dtype=torch.float64, device=dev)
    nb_o = lib.query("adnm_valid_objects_accum_ws_bytes", B * T, T, S, S, n)
    ws_o = torch.empty(max(nb_o, 16), dtype=torch.uint8, device=dev)
    table = torch.zeros(lib.query("adnm_valid_tracks_block_bytes", T, n) // 8, dtype=torch.float64, device=dev)
    nb = lib.query("adnm_valid_tracks_accum_ws_bytes", B * T, T, S, S, n)
    ws_t = torch.empty(nb, dtype=torch.uint8, device=dev)
    events, facts = {}, {}
    for name, (tg, pred) in field_pairs().items():
        tg, pred = tg.to(dev).contiguous(), pred.to(dev).contiguous()
        st = ops.track_stats(tg, pred, THR, SCALE).sum(dim=0)
        facts[name] = {"event_fraction_target_at_20": round(float(st[0, 0, 1]) / (B * T * S * S), 4), "tracks_per_sample_target_at_20": round(float(st[0, 0, 0]) / B, 2),
                       "mean_duration_target_at_20": round(float(st[0, 0, 3]) / max(float(st[0, 0, 0]), 1.0), 2), "spanning_target_at_20": int(st[0, 0, 6])}
        events[name] = {
            "adnm_valid_accum": event_ms(lambda: lib.call("adnm_valid_accum", pred.data_ptr(), tg.data_ptr(), block.data_ptr(), None, thr_c, n, SCALE, 0.57, 0.25,
                                                          0.0, ws.data_ptr(), ws.numel(), B * T, T, S * S, stream)),
            "adnm_valid_objects_accum": event_ms(lambda: lib.call("adnm_valid_objects_accum", pred.data_ptr(), T * S * S, S * S, tg.data_ptr(), table_o.data_ptr(), thr_c,
                                                                  n, SCALE, 1, ws_o.data_ptr(), nb_o, B * T, T, S, S, stream)),
            "adnm_valid_tracks_accum": event_ms(lambda: lib.call("adnm_valid_tracks_accum", pred.data_ptr(), T * S * S, S * S, tg.data_ptr(), table.data_ptr(), thr_c,
                                                                 n, SCALE, 1, ws_t.data_ptr(), nb, B * T, T, S, S, stream))}
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
lines.append(f"one call on the same tensors ({B} samples of {T}x{S}x{S}, {n} thresholds: {B * n * 2} chains, {B * T * n} labelling workgroups; forecast + target = {mb:.2f} MB; "
             f"tracks table {table.numel() * 8} bytes, workspace {nb} bytes), HIP events, every launch of the entry point, median (min .. max) of 20:")
for name, ev in events.items():
    lines.append(f"  {name}: {json.dumps(facts[name])}")
    for k, (m, lo, hi) in ev.items():
        lines.append(f"    {k:28s} {1e3 * m:8.1f} us  ({1e3 * lo:.1f} .. {1e3 * hi:.1f})")
    lines.append(f"    tracks / objects = {ev['adnm_valid_tracks_accum'][0] / ev['adnm_valid_objects_accum'][0]:.2f}   tracks / adnm_valid_accum = "
                 f"{ev['adnm_valid_tracks_accum'][0] / ev['adnm_valid_accum'][0]:.2f}   tracks / plain Validator.step = {ev['adnm_valid_tracks_accum'][0] / med['plain']:.3f}")
tr = results["tracks"]["tracks"]
lines.append("checks: " + json.dumps({"plain_keys_unchanged": repr({k: results['tracks'][k] for k in results['plain']}) == repr(results["plain"]),
                                      "target_volume_equals_TP_plus_FN": all(tr[v]["target"]["volume"] == int(results["tracks"]["threshold_metrics"][v]["TP"]
                                                                                                           + results["tracks"]["threshold_metrics"][v]["FN"]) for v in THR),
                                      "tracks_at_20": {k: tr[20][k] for k in ("count_bias", "duration_bias", "track_POD", "track_FAR", "track_CSI")},
                                      "target_at_20": {k: tr[20]["target"][k] for k in ("count", "per_sample", "mean_volume", "mean_duration", "initial", "spanning")},
                                      "survival_target_at_20": [round(float(v), 4) for v in tr[20]["target"]["survival"]],
                                      "survival_forecast_at_20": [round(float(v), 4) for v in tr[20]["forecast"]["survival"]]}))
text = "\n".join(lines)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
