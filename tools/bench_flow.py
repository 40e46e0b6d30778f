#!/usr/bin/env python3
"""What the flow advection costs beside the block scheme, for the record (profiles/flow_bench.txt): config 2 (ADNM-UNet 5 -> 20,
128 x 128, batch 4, T = 20, bf16), ONE session, one model.
  1. Validator.step for three configurations, the legs interleaved (a b c a b c ...), median and spread of 5 windows of N steps each,
     a host clock around work that ends in a device synchronise:
       plain         Validator(...)                                                   the baseline
       block         advection=True, fss=(1, 5, 17, 33), pools=(4, 16)                 trec_cost, trec_pick, advect, one pooled and one FSS pass
       flow          the same plus advection_flow=True                                trec_cost, trec_flow, advect_flow, the same two passes
  2. the HIP-event time of one adnm_trec_flow, adnm_flow_field and adnm_advect_flow call beside adnm_trec_motion and adnm_advect on the
     model's input, median of 20 after a warm-up, and each launch (trec_cost, trec_pick, trec_flow, advect, advect_flow, flow_field)
     alone from the library's own per-kernel events.
Run on the GPU box, under a time limit: timeout 600 python tools/bench_flow.py [--steps 16 --out profiles/flow_bench.txt]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_bench.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_flow.py: no GPU (a timing without one would mean nothing)")
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
        "block": Validator(model, crit, T, SCALE, THR, fss=FSS, pools=POOLS, advection=True),
        "flow": Validator(model, crit, T, SCALE, THR, fss=FSS, pools=POOLS, advection=True, advection_flow=True)}


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
    # the launches on the model's input, outside any graph
    block, radius, echo = legs["flow"].advection
    xin = x.reshape(B, 5, S, S)
    prev, last, stride, stream = xin.data_ptr() + 4 * 3 * S * S, xin.data_ptr() + 4 * 4 * S * S, 5 * S * S, torch.cuda.current_stream().cuda_stream
    nb = -(-S // block)
    ws = torch.empty(lib.query("adnm_trec_flow_ws_bytes", B, S, S, block, radius), dtype=torch.uint8, device=dev)
    motion, flow = (torch.zeros((B, nb, nb, 2), dtype=torch.int32, device=dev) for _ in range(2))
    field = torch.empty((B, S, S, 2), dtype=torch.int32, device=dev)
    out = torch.empty((B, T, S, S), dtype=torch.float32, device=dev)
    calls = {
        f"adnm_trec_motion (trec_cost + trec_pick), block {block} radius {radius}":
            lambda: lib.call("adnm_trec_motion", prev, last, stride, motion.data_ptr(), None, SCALE, block, radius, echo, ws.data_ptr(), ws.numel(), B, S, S, stream),
        f"adnm_trec_flow (trec_cost + trec_flow), block {block} radius {radius}":
            lambda: lib.call("adnm_trec_flow", prev, last, stride, flow.data_ptr(), None, SCALE, block, radius, echo, ws.data_ptr(), ws.numel(), B, S, S, stream),
        f"adnm_advect, block {block}, T {T}": lambda: lib.call("adnm_advect", last, stride, motion.data_ptr(), out.data_ptr(), block, B, T, S, S, stream),
        f"adnm_advect_flow, block {block}, T {T}": lambda: lib.call("adnm_advect_flow", last, stride, flow.data_ptr(), out.data_ptr(), block, B, T, S, S, stream),
        f"adnm_flow_field, block {block}": lambda: lib.call("adnm_flow_field", flow.data_ptr(), field.data_ptr(), block, B, S, S, stream)}
    events = {k: event_ms(fn) for k, fn in calls.items()}
    # each launch alone: the library's own per-kernel events (include/adnm_hip.h: adnm_prof_*), 20 calls
    lib.query("adnm_prof_enable", 1)
    for _ in range(20):
        for fn in calls.values():
            fn()
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
lines.append(f"  flow over block {med['flow'] - med['block']:+.3f} ms; block over plain {med['block'] - med['plain']:+.3f} ms")
lines.append(f"one call on the model's input ({B} samples of {S}x{S}; the transport writes {4.0 * B * T * S * S / 1e6:.2f} MB), HIP events, median (min .. max) of 20:")
for k, (m, lo, hi) in events.items():
    lines.append(f"  {k:70s} {1e3 * m:8.1f} us  ({1e3 * lo:.1f} .. {1e3 * hi:.1f})")
lines.append(f"each launch alone, block {block} radius {radius}, mean of the library's per-kernel events:")
for k in (k for k in ("trec_cost", "trec_pick", "trec_flow", "advect", "advect_flow", "flow_field") if k in kernels):
    lines.append(f"  {k:70s} {1e3 * kernels[k][1] / kernels[k][0]:8.1f} us  ({kernels[k][0]} launches)")
a_flow, a_block = results["flow"]["advection"], results["block"]["advection"]
lines.append("checks: " + json.dumps({"other_keys_unchanged": repr({k: v for k, v in results["flow"].items() if k != "advection"})
                                      == repr({k: v for k, v in results["block"].items() if k != "advection"}),
                                      "scheme": a_flow.get("scheme"),
                                      "flow_CSI": {str(t): a_flow["threshold_metrics"][t]["CSI"] for t in THR},
                                      "block_CSI": {str(t): a_block["threshold_metrics"][t]["CSI"] for t in THR}}))
text = "\n".join(lines)
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text + "\n")
