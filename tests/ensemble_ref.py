"""The CPU yardstick of the ensemble kernels (csrc/ensemble.hip; validate.ensemble_entries), written differently from them: the fields
are quantised with numpy in float32 (NaN put to 0 first, as fmaxf does), S2 comes from the full matrix np.abs(x[:, None] - x[None]), every
count from boolean masks and np.bincount, the members from torch.flip / transpose, the mean from a np.float32 loop.  Nothing is packed,
nothing is skipped for dry pixels: the table's convention (the dry pixels in Z alone) is applied at the very end by taking them out of
the bins they were counted in."""
import numpy as np
import torch


def quantise(v, scale):
    """fp32 field -> int64 levels 0 .. floor(scale): floor(clip(v, 0, 1) * scale) in float32; NaN -> 0 (fmaxf(NaN, 0) = 0)"""
    v = np.asarray(v, dtype=np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.floor(np.clip(v, np.float32(0), np.float32(1)) * np.float32(scale)).astype(np.int64)


def cols(M, nthr):
    return 7 + (M + 1) ** 2 + 2 * nthr * (M + 1)


# ------------------------------------------------------------------------------------------------ the symmetries of the square
def g(w, code):
    """torch (..., H, W) -> the member: flip up-down (bit 1), flip left-right (bit 0), transpose (bit 2), in that order"""
    if code & 2:
        w = w.flip(-2)
    if code & 1:
        w = w.flip(-1)
    if code & 4:
        w = w.transpose(-1, -2)
    return w.contiguous()


def g_inv(w, code):
    """the inverse: transpose first, then the flips"""
    if code & 4:
        w = w.transpose(-1, -2)
    if code & 1:
        w = w.flip(-1)
    if code & 2:
        w = w.flip(-2)
    return w.contiguous()


def members(x, codes, inverse=False):
    """x: torch (..., H, W), or (M, ..., H, W) with inverse -> (M, ..., H, W)"""
    return torch.stack([g_inv(x[m], c) if inverse else g(x, c) for m, c in enumerate(codes)])


# ------------------------------------------------------------------------------------------------ the score
def frame_rows(target, mem, thresholds, scale):
    """target (frames, ...) and mem (M, frames, ...) float32 -> (frames, C) int64, the kernel's table with T = frames"""
    y, x = quantise(target, scale), quantise(mem, scale)
    M, frames = x.shape[0], y.shape[0]
    y, x = y.reshape(frames, -1), x.reshape(M, frames, -1)
    out = np.zeros((frames, cols(M, len(thresholds))), dtype=np.int64)
    for f in range(frames):
        yy, xx = y[f], x[:, f]
        dry = (yy == 0) & (xx == 0).all(axis=0)
        sx = xx.sum(axis=0)
        out[f, 0] = yy.size
        out[f, 1] = dry.sum()
        out[f, 2] = np.abs(xx[0] - yy).sum()
        out[f, 3] = np.abs(xx - yy).sum()
        out[f, 4] = np.abs(xx[:, None] - xx[None]).sum() // 2      # every pair twice, the diagonal zero
        out[f, 5] = (M * (xx * xx).sum(axis=0) - sx * sx).sum()
        out[f, 6] = ((sx - M * yy) ** 2).sum()
        below, equal = (xx < yy).sum(axis=0), (xx == yy).sum(axis=0)
        rank = np.bincount((below * (M + 1) + equal)[~dry], minlength=(M + 1) ** 2)
        out[f, 7:7 + (M + 1) ** 2] = rank
        at = 7 + (M + 1) ** 2
        for k, thr in enumerate(thresholds):
            o, c = (yy.astype(np.float32) >= np.float32(thr)).astype(np.int64), (xx.astype(np.float32) >= np.float32(thr)).sum(axis=0)
            out[f, at + 2 * k * (M + 1):at + 2 * (k + 1) * (M + 1)] = np.bincount((o * (M + 1) + c)[~dry], minlength=2 * (M + 1))
    return out


def table(target, mem, thresholds, scale, T):
    """-> (T, C) int64: frame f belongs to row f mod T"""
    rows = frame_rows(target, mem, thresholds, scale)
    out = np.zeros((T, rows.shape[1]), dtype=np.int64)
    for f in range(rows.shape[0]):
        out[f % T] += rows[f]
    return out


def crps_integral(target, mem, scale):
    """M^2 N crps as the integral of the squared CDF difference over the levels: SUM_px SUM_{l=0}^{Q-1} (#{x_i <= l} - M [y <= l])^2"""
    y, x = quantise(target, scale).ravel(), quantise(mem, scale).reshape(np.shape(mem)[0], -1)
    M, Q = x.shape[0], int(np.floor(np.float32(scale)))
    total = 0
    for lev in range(Q):
        total += int((((x <= lev).sum(axis=0) - M * (y <= lev)) ** 2).sum())
    return total


def s2_sorted(mem, scale):
    """S2 = SUM_i (2 i - M - 1) x_(i) on the sorted members, i = 1 .. M"""
    x = np.sort(quantise(mem, scale).reshape(np.shape(mem)[0], -1), axis=0)
    M = x.shape[0]
    w = 2 * np.arange(1, M + 1) - M - 1
    return int((w[:, None] * x).sum())


# ------------------------------------------------------------------------------------------------ the product
def product(mem, thresholds, scale):
    """mem (M, ...) float32 -> (mean, prob): the np.float32 loop and np.float32(c) / np.float32(M)"""
    mem = np.asarray(mem, dtype=np.float32)
    M = mem.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        s = mem[0].copy()
        for i in range(1, M):
            s = (s + mem[i]).astype(np.float32)
        mean = (s / np.float32(M)).astype(np.float32)
    if not len(thresholds):
        return mean, None
    q = quantise(mem, scale).astype(np.float32)
    prob = np.stack([(q >= np.float32(t)).sum(axis=0).astype(np.float32) / np.float32(M) for t in thresholds]).astype(np.float32)
    return mean, prob


# ------------------------------------------------------------------------------------------------ fields
def blobs(rng, frames, H, W):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fld = np.zeros((frames, H, W))
    for i in range(frames):
        for _ in range(2):
            cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.8, 0.12 * max(H, W) + 1.0)
            fld[i] += rng.uniform(0.3, 1.3) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    return fld


def radar_stack(M, frames, H, W, seed, plant=True):
    """-> (target (frames, H, W), members (M, frames, H, W)) float32: about 90 % exact zeros, the members perturbed copies of one field that
    is itself a shifted, weaker copy of the target; with `plant` NaN, +-Inf, negatives and values > 1 in target and members"""
    rng = np.random.default_rng(seed)
    base = blobs(rng, frames, H, W)
    cut = np.quantile(base, 0.9) if base.size > 1 else 0.5
    tgt = np.where(base < cut, 0.0, base).astype(np.float32)
    mem = np.empty((M, frames, H, W), dtype=np.float32)
    for m in range(M):
        f = np.roll(base, m % 3, axis=-1) * rng.uniform(0.7, 1.1) + rng.normal(0.0, 0.02, base.shape)
        mem[m] = np.where(f < cut, 0.0, f)
    if plant:
        for arr, off in ((tgt, 0), (mem, 5)):
            flat = arr.reshape(-1)
            for k, bad in enumerate((np.nan, np.inf, -np.inf, -0.25, 1.75, np.nan, 1.0)):
                flat[(k * 7919 + off + seed) % flat.size] = bad
    return tgt, mem


def noise_stack(M, frames, H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.02, 1.02, (frames, H, W)).astype(np.float32), rng.uniform(-0.02, 1.02, (M, frames, H, W)).astype(np.float32)
