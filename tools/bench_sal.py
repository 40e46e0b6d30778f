#!/usr/bin/env python3
"""What the SAL scores cost, for the record (profiles/sal_bench.txt): config 2 (ADNM-UNet 5 -> 20, 128 x 128, batch 4, T = 20, bf16), the
reference's four thresholds, ONE session, one model.
  1. Validator.step for two configurations, the legs interleaved (a b a b ...), median and spread of 5 windows of N steps each, a host
     clock around work that ends in a device synchronise:
       plain         Validator(...)                                   the parent's behaviour, the baseline
       sal           sal=True
  2. the HIP-event time of one adnm_valid_sal_accum call (both launches) beside one adnm_valid_objects_accum call and one adnm_valid_accum
     call on the same tensors, median of 20 after a warm-up, for three pairs of fields:
       zero          both fields all zero: staging the bits and the bytes and the empty passes alone
       sparse        smooth blobs over about 90 % zeros, the forecast a blurred, shifted copy: what a radar field looks like
       noise41       independent noise with 41 % events at every threshold: around the 8-connected percolation point, the most tangled shapes
     No time is fixed in advance: the objects pass of the same session is the comparison, because it does the same labelling.
  3. where the time goes: the objects call and the SAL call on B * T frames of independent noise (41 %, 10 %, none) at 112, 128, 168 and 256
     pixels a side, one frame size per place the records and the words of the SAL pass can live (112: both in LDS; 128 and 168: the records
     in the workspace; 256: both in the workspace, as the objects pass's words are), with the bytes of the SAL pass's workspace slices.
Run on the GPU box, under a time limit: timeout 600 python tools/bench_sal.py [--steps 16 --out profiles/sal_bench.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sal_bench.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_sal.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
THR, SCALE, T, S, B = (20, 30, 35, 40), 90.0, 20, args.size, args.batch
model = create_ADNMUNet(5, T, 6, img_size=S)
recipe.fill_parameters(model)
model = model.to(dev).eval()
crit = enRainfallLoss(0.57, 0.25, gamma=0.0)
frames = recipe.radar_batch(B, 25, S, name="bench").to(dev)
x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
ops.set_mfma_precision(args.dtype)
legs = {"plain": Validator(model, crit, T, SCALE, THR), "sal": Validator(model, crit, T, SCALE, THR, sal=True)}


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
    return {"zero": (zero, zero.clone()), "sparse": (sparse_t, sparse_f),
            "noise41": ((torch.rand(n, S, S, generator=g) < 0.41).float(), (torch.rand(n, S, S, generator=g) < 0.41).float())}


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
    table_s = torch.zeros(lib.query("adnm_valid_sal_block_bytes", T, n) // 8, dtype=torch.float64, device=dev)
    nb_s = lib.query("adnm_valid_sal_accum_ws_bytes", B * T, T, S, S, n)
    ws_s = torch.empty(nb_s, dtype=torch.uint8, device=dev)
    events, facts = {}, {}
    for name, (tg, pred) in field_pairs().items():
        tg, pred = tg.to(dev).contiguous(), pred.to(dev).contiguous()
        st = ops.object_stats(tg, pred, THR, SCALE)
        rows = ops.sal_table(tg, pred, THR, SCALE).sum(dim=0)[0].tolist()
        facts[name] = {"event_fraction_target_at_20": round(float(st[:, 0, 0, 1].sum()) / (B * T * S * S), 4),
                       "objects_per_frame_target_at_20": round(float(st[:, 0, 0, 0].sum()) / (B * T), 2),
                       "frames_with_S_at_20": int(rows[5]), "mean_S_at_20": round(rows[6] / rows[5], 4) if rows[5] else None}
        events[name] = {
            "adnm_valid_accum": event_ms(lambda: lib.call("adnm_valid_accum", pred.data_ptr(), tg.data_ptr(), block.data_ptr(), None, thr_c, n, SCALE, 0.57, 0.25,
                                                          0.0, ws.data_ptr(), ws.numel(), B * T, T, S * S, stream)),
            "adnm_valid_objects_accum": event_ms(lambda: lib.call("adnm_valid_objects_accum", pred.data_ptr(), T * S * S, S * S, tg.data_ptr(), table_o.data_ptr(), thr_c,
                                                                  n, SCALE, 1, ws_o.data_ptr(), nb_o, B * T, T, S, S, stream)),
            "adnm_valid_sal_accum": event_ms(lambda: lib.call("adnm_valid_sal_accum", pred.data_ptr(), T * S * S, S * S, tg.data_ptr(), table_s.data_ptr(), thr_c, n,
                                                              SCALE, 1, None, ws_s.data_ptr(), nb_s, B * T, T, S, S, stream))}
    # 3. the same two calls per place the records and the words can live
    sweep = []
    g = torch.Generator(device="cpu").manual_seed(7)
    for side in (112, 128, 168, 256):
        need_o = lib.query("adnm_valid_objects_accum_ws_bytes", B * T, T, side, side, n)
        slab_o = torch.empty(max(need_o, 16), dtype=torch.uint8, device=dev)
        need_s = lib.query("adnm_valid_sal_accum_ws_bytes", B * T, T, side, side, n)
        slab_s = torch.empty(need_s, dtype=torch.uint8, device=dev)
        for name, density in (("noise41", 0.41), ("noise10", 0.10), ("zero", 0.0)):
            tg = (torch.rand(B * T, side, side, generator=g) < density).float().to(dev)
            pred = (torch.rand(B * T, side, side, generator=g) < density).float().to(dev)
            t_o = event_ms(lambda: lib.call("adnm_valid_objects_accum", pred.data_ptr(), T * side * side, side * side, tg.data_ptr(), table_o.data_ptr(), thr_c, n,
                                          SCALE, 1, slab_o.data_ptr(), need_o, B * T, T, side, side, stream))[0]
            t_s = event_ms(lambda: lib.call("adnm_valid_sal_accum", pred.data_ptr(), T * side * side, side * side, tg.data_ptr(), table_s.data_ptr(), thr_c, n, SCALE,
                                          1, None, slab_s.data_ptr(), need_s, B * T, T, side, side, stream))[0]
            sweep.append(f"  {side:4d} x {side:<4d} {name:8s} objects {1e3 * t_o:8.1f} us   sal {1e3 * t_s:8.1f} us   sal / objects {t_s / t_o:.2f}   "
                         f"(slices {need_s - 8 * B * T * n * 12} bytes)")
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
lines.append(f"one call on the same tensors ({B * T} frames of {S}x{S}, {n} thresholds: {B * T * n} items; forecast + target = {mb:.2f} MB; SAL table "
             f"{table_s.numel() * 8} bytes, SAL workspace {nb_s} bytes, objects workspace {nb_o} bytes), HIP events, every launch of the entry point, "
             "median (min .. max) of 20:")
for name, ev in events.items():
    lines.append(f"  {name}: {json.dumps(facts[name])}")
    for k, (m, lo, hi) in ev.items():
        lines.append(f"    {k:28s} {1e3 * m:8.1f} us  ({1e3 * lo:.1f} .. {1e3 * hi:.1f})")
    lines.append(f"    sal / objects = {ev['adnm_valid_sal_accum'][0] / ev['adnm_valid_objects_accum'][0]:.2f}   sal / adnm_valid_accum = "
                 f"{ev['adnm_valid_sal_accum'][0] / ev['adnm_valid_accum'][0]:.2f}")
sal = results["sal"]["sal"]
lines.append("checks: " + json.dumps({"plain_keys_unchanged": repr({k: results['sal'][k] for k in results['plain']}) == repr(results["plain"]),
                                      "sal_at_20": {k: sal[20][k] for k in ("A", "S", "L1", "L2", "L", "frames_A", "frames_S", "missed_frames", "false_frames")}}))
lines.append(f"where the time goes: one adnm_valid_objects_accum and one adnm_valid_sal_accum call on {B * T} frames of independent noise (41 %, 10 %, none), {n} thresholds, "
             "HIP events, median of 20, at one frame size per place the records and the words of the SAL pass can live (112: both in LDS; 128 and 168: the records in "
             "the workspace; 256: both in the workspace, as the objects pass's words are):")
lines += sweep
text = "\n".join(lines)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
