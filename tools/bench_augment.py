#!/usr/bin/env python3
"""For the record: what augmentation in the fetch costs, on bench.py's workload (ADNM-UNet 5 -> 20, FlatTrainer hipGraph
replay, 128 x 128, batch 4, 25 frames), everything in one session:
  launches  the device time of one launch of adnm_batch_fetch (the yardstick) and of adnm_batch_fetch_aug with five word sets, all into
            the trainer's static buffers: identity (all words 0), flips (codes 1, 2, 3 in turn), transposed (codes 4 .. 7 in turn: every
            sample goes through the LDS tile), crop160_ox1 (a 160 x 160 store, no symmetry, ox = 1 mod 4: every sample float by float),
            random (the 160 x 160 store, Augment(seed=0)'s own words: all paths in one launch).  Each figure is the mean over 50 launches
            captured in one graph and replayed 200 times between two HIP events; the variants are measured in turn, 5 rounds, and the
            median and all rounds are printed, so that the spread of the yardstick is there to compare a difference with.
  steps     ms per step of FlatTrainer.step_from over a plain feed (128 x 128 store) and over an augmenting feed (160 x 160 store,
            crop=(128, 128), Augment(seed=0)) on ONE prepared trainer, in alternating windows (wall clock between device
            synchronisations), 5 windows each.
The stores are seeded random fields made on the device (the fetch moves bit patterns: their values do not matter).  One JSON line.
Run on the GPU box: python tools/bench_augment.py [--steps 40 --warmup 8 --samples 32 --dtype bf16]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import torch
from adnm_hip import lib, ops, recipe
from adnm_hip.dataio import Augment, ResidentDataset, pack_word
from adnm_hip.trainer import FlatTrainer
from models.ADNMUNet import create_ADNMUNet
from models.loss import enRainfallLoss

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40, help="timed steps per window (5 windows per feed)")
ap.add_argument("--warmup", type=int, default=8, help="warm-up steps per feed")
ap.add_argument("--samples", type=int, default=32)
ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16", "fp8"])
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_augment.py: no GPU (a timing without one would mean nothing)")
dev = torch.device("cuda", 0)
ops.set_mfma_precision(args.dtype)
os.environ["ADNM_AUTO_DDP"] = "0"
N, B, S, BIG, T, T_IN, ROUNDS = args.samples, 4, 128, 160, 25, 5, 5

gen = torch.Generator(device=dev).manual_seed(0)
store = torch.rand((N, T, S, S), device=dev, generator=gen) * (70.0 / 255.0)
big = torch.rand((N, T, BIG, BIG), device=dev, generator=gen) * (70.0 / 255.0)
plain = ResidentDataset(store, T_IN, B, generator=torch.Generator().manual_seed(1))
augmenting = ResidentDataset(big, T_IN, B, generator=torch.Generator().manual_seed(1), crop=(S, S), augment=Augment(seed=0))

model = create_ADNMUNet(5, 20, 6, img_size=S)
recipe.fill_parameters(model)
model = model.to(dev).train()
tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0).to(dev), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                 use_graph=True)
frames = recipe.radar_batch(B, T, S, name="bench").to(dev)
tr.prepare(frames[:, :T_IN].contiguous(), frames[:, T_IN:].contiguous())


# ---- steps: alternating windows on one trainer
def run(feed, n):
    for _ in range(n):
        if feed.order.perm is None or feed.order.pos == len(feed):
            feed.begin_epoch()
        tr.step_from(feed)


feeds = [("plain", plain), ("augment", augmenting)]
for _, feed in feeds:
    run(feed, args.warmup)
torch.cuda.synchronize()
windows = {name: [] for name, _ in feeds}
for _ in range(ROUNDS):
    for name, feed in feeds:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(feed, args.steps)
        torch.cuda.synchronize()
        windows[name].append(1e3 * (time.perf_counter() - t0) / args.steps)

# ---- launches: the raw entry points into the trainer's static buffers
order = torch.randperm(N, generator=torch.Generator().manual_seed(2)).to(torch.int32).to(dev)
k = torch.arange(N)
rnd = torch.Generator().manual_seed(3)
word_sets = {
    "identity": (store, torch.zeros(N, dtype=torch.int32)),
    "flips": (store, pack_word(1 + k % 3, 0 * k, 0 * k)),
    "transposed": (store, pack_word(4 + k % 4, 0 * k, 0 * k)),
    "crop160_ox1": (big, pack_word(0 * k, torch.randint(0, BIG - S + 1, (N,), generator=rnd), 1 + 4 * torch.randint(0, (BIG - S) // 4, (N,), generator=rnd))),
    "random": (big, Augment(seed=0).draw(N, BIG - S, BIG - S)),
}
word_sets = {name: (st, w.to(dev)) for name, (st, w) in word_sets.items()}
stream = lambda: torch.cuda.current_stream(dev).cuda_stream
steps_per_epoch = N // B


def launch_plain(i):
    lib.call("adnm_batch_fetch", store.data_ptr(), N, T, S * S, order.data_ptr(), N, (i % steps_per_epoch) * B, tr.sx.data_ptr(), tr.st.data_ptr(), B, T_IN,
             stream())


def launch_aug(name):
    st, words = word_sets[name]

    def fn(i):
        lib.call("adnm_batch_fetch_aug", st.data_ptr(), N, T, st.shape[2], st.shape[3], order.data_ptr(), words.data_ptr(), N, (i % steps_per_epoch) * B,
                 tr.sx.data_ptr(), tr.st.data_ptr(), B, T_IN, S, S, stream())
    return fn


def graph_of(fn, per_graph=50):
    fn(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(per_graph):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    return g, per_graph


def device_us(graph, replays=200):
    g, per_graph = graph
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / (per_graph * replays)


graphs = [("plain", graph_of(launch_plain))] + [(name, graph_of(launch_aug(name))) for name in word_sets]
rounds = {name: [] for name, _ in graphs}
for _ in range(ROUNDS):
    for name, g in graphs:
        rounds[name].append(device_us(g))

out = {"metric": f"ADNM-UNet 5->20 {S}x{S} batch {B} {args.dtype}: adnm_batch_fetch against adnm_batch_fetch_aug, {N} samples of {T} frames, stores {S}x{S} and {BIG}x{BIG}",
       "steps_per_window": args.steps, "bytes_per_launch": 8 * B * T * S * S}
base = statistics.median(rounds["plain"])
for name, _ in graphs:
    out[f"launch_us_{name}"] = round(statistics.median(rounds[name]), 2)
    out[f"rounds_us_{name}"] = [round(v, 2) for v in rounds[name]]
    if name != "plain":
        out[f"ratio_{name}"] = round(statistics.median(rounds[name]) / base, 3)
for name, _ in feeds:
    out[f"ms_per_step_{name}"] = round(statistics.median(windows[name]), 3)
    out[f"windows_{name}"] = [round(v, 3) for v in windows[name]]
print(json.dumps(out))
tr.close()
