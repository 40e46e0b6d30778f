"""The CPU yardstick of the Fractions Skill Score sums (csrc/neighbour.hip: adnm_valid_fss_accum): the fields quantised the way
adnm_eval_counts quantises them (verify_ref.quant), thresholded, and counted per n x n window centred on every pixel with zero padding
by conv2d of the float64 bit fields with an all-ones kernel (exact integers).  Per frame, scale and threshold A = sum c_o^2,
F = sum c_f^2, C = sum c_o c_f; FSS = 2C / (A + F).  Sums are integers: every comparison against this reference is exact.  The reference
project has no FSS, so nothing here is recorded from it."""
import numpy as np
import torch
import torch.nn.functional as F

import verify_ref as R

THR_SETS, SCALE = R.THR_SETS, R.SCALE
SCALES = (1, 3, 9, 17, 33)
# (frames, H, W, seed) of verify_ref.radar_fields: each is dense (assert_dense) at the one- and four-threshold sets for every scale of SCALES
CASES = [(8, 64, 64, 0), (6, 37, 53, 1), (4, 128, 128, 2), (3, 33, 33, 3), (2, 5, 40, 4), (2, 16, 16, 5)]


def window_counts(bits, n):
    """bits: (frames, H, W) float64 of 0 / 1 -> the number of ones in the n x n window centred on every pixel, zeros outside the frame"""
    x = torch.from_numpy(np.ascontiguousarray(bits, dtype=np.float64))[:, None]
    return F.conv2d(x, torch.ones((1, 1, n, n), dtype=torch.float64), padding=n // 2)[:, 0].numpy()


def ref_sums(truth, pred, thresholds, scale, scales):
    """truth, pred: (frames, H, W) float arrays -> (frames, nscale, 3 * nthr) float64: A, F, C per threshold"""
    qt, qp = R.quant(np.asarray(truth), scale), R.quant(np.asarray(pred), scale)
    out = np.zeros((qt.shape[0], len(scales), 3 * len(thresholds)), dtype=np.float64)
    for k, thr in enumerate(thresholds):
        o, f = (qt >= np.float32(thr)).astype(np.float64), (qp >= np.float32(thr)).astype(np.float64)
        for i, n in enumerate(scales):
            co, cf = window_counts(o, n), window_counts(f, n)
            assert (co == np.rint(co)).all() and (cf == np.rint(cf)).all()
            out[:, i, 3 * k + 0] = (co * co).sum(axis=(1, 2))
            out[:, i, 3 * k + 1] = (cf * cf).sum(axis=(1, 2))
            out[:, i, 3 * k + 2] = (co * cf).sum(axis=(1, 2))
    return out


def loop_sums(truth, pred, thresholds, scale, scales):
    """the same by a plain double loop over the windows (the helper's self-check: small cases only)"""
    qt, qp = R.quant(np.asarray(truth), scale), R.quant(np.asarray(pred), scale)
    frames, H, W = qt.shape
    out = np.zeros((frames, len(scales), 3 * len(thresholds)), dtype=np.float64)
    for i, n in enumerate(scales):
        r = n // 2
        for f in range(frames):
            for y in range(H):
                for x in range(W):
                    wt, wp = (q[f, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] for q in (qt, qp))
                    for k, thr in enumerate(thresholds):
                        co, cf = int((wt >= thr).sum()), int((wp >= thr).sum())
                        out[f, i, 3 * k:3 * k + 3] += (co * co, cf * cf, co * cf)
    return out


def fss(sums):
    """(..., 3 * nthr) -> (..., nthr): 2C / (A + F) in double, NaN where A + F = 0"""
    sums = np.asarray(sums, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 * sums[..., 2::3] / (sums[..., 0::3] + sums[..., 1::3])


def radar_fields(frames, H, W, seed):
    return R.radar_fields(frames, H, W, seed)


def assert_dense(ref, what=""):
    """a test may hide a failure by scoring only empty cells or a perfect / hopeless forecast: summed over the frames every A, F and C is
    > 0 and every FSS lies strictly between 0.05 and 0.98.  -> (smallest, largest) FSS"""
    cells = ref.sum(axis=0)
    score = fss(cells)
    assert (cells > 0).all(), f"{what}: a sum of the CPU reference is empty (smallest {cells.min()}): pick another seed, do not weaken this"
    assert (score > 0.05).all() and (score < 0.98).all(), \
        f"{what}: FSS of the CPU reference in [{score.min():.3f}, {score.max():.3f}], not inside (0.05, 0.98): pick another seed, do not weaken this"
    return float(score.min()), float(score.max())
