#!/usr/bin/env python3
"""For the record: what feeding the training step costs, by route, on bench.py's workload (ADNM-UNet 5 -> 20, FlatTrainer hipGraph
replay) with N synthetic samples of 25 byte frames of 565 x 784 (the Shanghai files' size), all routes in one session on ONE prepared
trainer, windows interleaved, ms per step = the median of 3 windows (wall clock between device synchronisations: most of what differs
between the routes is host work that no HIP event sees):
  (0) device  step(x, tgt) on batches that already lie on the device (N / B of them, cut from the same store, taken in turn): no feed
              at all; what step() then does is its two device copies into the graph's static buffers;
  (a) host    the reference's route (train.py:44-57,132-134): float samples at S x S in host memory, collated per step, .to(device);
  (b) ingest  dataio.RadarIngest.submit / take (the next batch's bytes are submitted before this batch's step) + step(x, tgt);
  (c) feed    dataio.ResidentDataset (built once with from_bytes: its time is printed) + FlatTrainer.step_from.
Every feeding route draws its batches in the same EpochOrder.  Beside the step times: the device time of one fetch launch and of the two
copies it replaces, each as the mean over 50 launches captured in one graph and replayed 20 times between two HIP events.  One JSON line.
Run on the GPU box: python tools/bench_feed.py [--steps 40 --warmup 8 --samples 32 --batch 4 --size 128 --dtype bf16]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import torch
from adnm_hip import ops, recipe
from adnm_hip.dataio import EpochOrder, RadarIngest, ResidentDataset
from adnm_hip.trainer import FlatTrainer
from models.ADNMUNet import create_ADNMUNet
from models.loss import enRainfallLoss

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40, help="timed steps per window (3 windows per route)")
ap.add_argument("--warmup", type=int, default=8, help="warm-up steps per route")
ap.add_argument("--samples", type=int, default=32)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16", "fp8"])
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_feed.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
ops.set_mfma_precision(args.dtype)
os.environ["ADNM_AUTO_DDP"] = "0"
N, B, S, T, T_IN, H0, W0 = args.samples, args.batch, args.size, 25, 5, 565, 784

raw = torch.randint(0, 71, (N, T, H0, W0), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
torch.cuda.synchronize()
t0 = time.perf_counter()
feed = ResidentDataset.from_bytes(raw, S, T_IN, B, dev, generator=torch.Generator().manual_seed(1))
torch.cuda.synchronize()
build_ms = 1e3 * (time.perf_counter() - t0)
host = [s.unsqueeze(1).contiguous() for s in feed.store.cpu()]        # route (a): the list datasets/Shanghai.py builds at import
raw_np = raw.numpy()

model = create_ADNMUNet(5, 20, 6, img_size=S)
recipe.fill_parameters(model)
model = model.to(dev).train()
tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0).to(dev), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                 use_graph=True)
frames = recipe.radar_batch(B, T, S, name="bench").to(dev)
x0, t0_ = frames[:, :T_IN].contiguous(), frames[:, T_IN:].contiguous()
tr.prepare(x0, t0_)
ingest = RadarIngest(B, T, H0, W0, S, dev, in_frames=T_IN)


def batches(order, n):
    """the index lists of the next n batches, epoch after epoch"""
    for _ in range(n):
        if order.perm is None or order.pos == len(order):
            order.next_epoch()
        yield order.next_batch().tolist()


resident = [(feed.store[i:i + B, :T_IN].unsqueeze(2).contiguous(), feed.store[i:i + B, T_IN:].unsqueeze(2).contiguous()) for i in range(0, N - B + 1, B)]
turn = [0]


def run_device(n, order):
    for _ in range(n):
        x, tgt = resident[turn[0] % len(resident)]
        turn[0] += 1
        tr.step(x, tgt)


def run_host(n, order):
    for idx in batches(order, n):
        data = torch.stack([host[i] for i in idx])                    # the default collate
        tr.step(data[:, :T_IN].to(dev), data[:, T_IN:].to(dev))


def run_ingest(n, order):
    it = batches(order, n)
    ingest.submit(raw_np[next(it)])
    for k in range(n):
        x, tgt = ingest.take()
        if k + 1 < n:
            ingest.submit(raw_np[next(it)])
        tr.step(x, tgt)


def run_feed(n, order):
    for _ in range(n):
        if feed.order.perm is None or feed.order.pos == len(feed):
            feed.begin_epoch()
        tr.step_from(feed)


routes = [("device", run_device), ("host", run_host), ("ingest", run_ingest), ("feed", run_feed)]
orders = {name: EpochOrder(N, B, generator=torch.Generator().manual_seed(1)) for name, _ in routes}
for name, fn in routes:
    fn(args.warmup, orders[name])
torch.cuda.synchronize()
windows = {name: [] for name, _ in routes}
for _ in range(3):
    for name, fn in routes:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(args.steps, orders[name])
        torch.cuda.synchronize()
        windows[name].append(1e3 * (time.perf_counter() - t0) / args.steps)


def device_us(fn, per_graph=50, replays=20):
    """device time of fn's launches without the host between them: per_graph calls captured in one graph, replayed between two events"""
    fn(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(per_graph):
            fn(k)
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / (per_graph * replays)


def one_fetch(k):
    feed.order.pos = k % len(feed)
    feed.fetch_into(tr.sx, tr.st)


def two_copies(k):
    x, tgt = resident[k % len(resident)]
    tr.sx.copy_(x, non_blocking=True)
    tr.st.copy_(tgt, non_blocking=True)


feed.begin_epoch()
torch.cuda.synchronize()
fetch_us, copies_us = device_us(one_fetch), device_us(two_copies)
out = {"metric": f"ADNM-UNet 5->20 {S}x{S} batch {B} {args.dtype} FlatTrainer graph replay, fed four ways; {N} samples of {T} x {H0} x {W0} bytes",
       "steps_per_window": args.steps, "store_bytes": feed.store_bytes, "store_build_ms": round(build_ms, 1),
       "fetch_device_us": round(fetch_us, 2), "two_copies_device_us": round(copies_us, 2)}
for name, _ in routes:
    w = windows[name]
    out[f"ms_per_step_{name}"] = round(statistics.median(w), 3)
    out[f"windows_{name}"] = [round(v, 3) for v in w]
print(json.dumps(out))
tr.close()
