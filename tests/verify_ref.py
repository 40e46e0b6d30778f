"""The CPU yardstick of the pooled contingency counts (csrc/neighbour.hip: adnm_valid_pool_accum): torch's max_pool2d applied to the fields
quantised the way adnm_eval_counts quantises them, and a generator of radar-like fields.  Counts are integers: every comparison against
this reference is exact.  The reference project has no pooled score, so nothing here is recorded from it."""
import numpy as np
import torch
import torch.nn.functional as F

THR = [20, 30, 35, 40]
THR_SETS = {"one": [30], "default": THR, "eight": [5, 10, 20, 30, 35, 40, 50, 70]}   # those of test_validate_gpu.py
SCALE = 90.0


def pairs(pools):
    return [tuple(p) if isinstance(p, (tuple, list)) else (p, p) for p in pools]


def quant(v, scale):
    """q(v) = floorf(fminf(fmaxf(v, 0), 1) * scale) in fp32, bit-equal to the device statement: fmaxf(NaN, 0) = 0, so NaN -> 0 (np.clip
    would keep it), -Inf -> 0, +Inf -> floor(scale); one fp32 multiply, one floor."""
    v = np.asarray(v, dtype=np.float32)
    c = np.clip(np.where(np.isnan(v), np.float32(0), v), np.float32(0), np.float32(1)).astype(np.float32)
    return np.floor(c * np.float32(scale)).astype(np.float32)


def windows(H, W, pool):
    s, d = pool
    return ((H - s) // d + 1) * ((W - s) // d + 1)


def ref_counts(truth, pred, thresholds, scale, pools):
    """truth, pred: (frames, H, W) float arrays -> (frames, npool, 4 * nthr) float64: TP, FN, FP, TN per threshold, counted per window of
    max_pool2d(kernel_size=s, stride=d, padding=0, ceil_mode=False) on the quantised fields"""
    qt, qp = (torch.from_numpy(quant(np.asarray(a), scale))[:, None] for a in (truth, pred))
    out = np.zeros((qt.shape[0], len(pools), 4 * len(thresholds)), dtype=np.float64)
    for i, (s, d) in enumerate(pairs(pools)):
        mt, mp = (F.max_pool2d(q, kernel_size=s, stride=d, padding=0, ceil_mode=False)[:, 0].numpy() for q in (qt, qp))
        for k, thr in enumerate(thresholds):
            o, f = mt >= np.float32(thr), mp >= np.float32(thr)
            for c, cell in enumerate((o & f, o & ~f, ~o & f, ~o & ~f)):
                out[:, i, 4 * k + c] = cell.sum(axis=(1, 2))
    return out


def loop_counts(truth, pred, thresholds, scale, pools):
    """the same by a plain any-over-window loop (the helper's self-check: small cases only)"""
    qt, qp = quant(np.asarray(truth), scale), quant(np.asarray(pred), scale)
    n, H, W = qt.shape
    out = np.zeros((n, len(pools), 4 * len(thresholds)), dtype=np.float64)
    for i, (s, d) in enumerate(pairs(pools)):
        for f in range(n):
            for y in range(0, H - s + 1, d):
                for x in range(0, W - s + 1, d):
                    for k, thr in enumerate(thresholds):
                        o, m = bool((qt[f, y:y + s, x:x + s] >= thr).any()), bool((qp[f, y:y + s, x:x + s] >= thr).any())
                        out[f, i, 4 * k + (0 if o and m else 1 if o else 2 if m else 3)] += 1
    return out


def blobs(rng, n, H, W, count):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((n, H, W), dtype=np.float64)
    for f in range(n):
        for _ in range(count):
            cy, cx, amp, sig = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.25, 0.62), rng.uniform(2.0, 6.0)
            out[f] += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sig * sig))
    return out


def radar_fields(n, H, W, seed):
    """-> (target, forecast), (n, H, W) fp32.  Uniform noise would make every pooled window an event and every test vacuous: the target is
    three Gaussian blobs per frame (amplitude 0.25-0.62, sigma 2-6 px); the forecast is 0.85 * roll(target, (2, -3)) plus one blob of its
    own plus N(0, 0.02) noise, so it is displaced, weaker, and leaves [0, 1] on both sides."""
    rng = np.random.default_rng(seed)
    tgt = blobs(rng, n, H, W, 3)
    pred = 0.85 * np.roll(tgt, (2, -3), axis=(1, 2)) + blobs(rng, n, H, W, 1) + rng.normal(0.0, 0.02, size=tgt.shape)
    return tgt.astype(np.float32), pred.astype(np.float32)


def assert_dense(ref, what=""):
    """a test may hide a failure by scoring only empty cells: on a dense case every one of TP, FN, FP, TN is > 0 for every threshold and
    pool (summed over the frames)"""
    cells = ref.sum(axis=0)
    assert (cells > 0).all(), f"{what}: a cell of the CPU reference is empty (smallest {cells.min()}): pick another seed, do not weaken this"
    return cells.min()
