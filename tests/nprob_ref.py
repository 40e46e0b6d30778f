"""The CPU yardstick of the neighbourhood exceedance probability (csrc/neighbour.hip: adnm_valid_nprob_accum, adnm_neighbour_prob;
validate.nprob_entries), written differently from both: the fields are quantised with numpy in float32 as joint_ref does it, the window
counts are conv2d of the float64 event mask with an all-ones kernel and padding n // 2, the table is np.bincount(c + (n^2 + 1) * o), and
every score comes from boolean masks and explicit sums over the PIXELS, not from the table.  The reference project has no such score, so
nothing here is recorded from it.  The module checks its window counts once, when it is imported, against scipy.ndimage.uniform_filter."""
import numpy as np
import torch
import torch.nn.functional as F

import joint_ref as J


def layout(scales):
    """-> ([(start of o = 0, start of o = 1)] per scale, S): written out here on its own, the test of ops.nprob_layout compares with it"""
    at, out = 0, []
    for n in scales:
        out.append((at, at + n * n + 1))
        at += 2 * (n * n + 1)
    return out, at


def events(field, thr, scale):
    """(frames, H, W) float field -> bool: the quantised value reaches thr"""
    return J.quantise(field, scale) >= thr


def window_counts(mask, n):
    """bool (frames, H, W) -> int64: the events in the n x n window centred on every pixel, zeros outside the frame"""
    x = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.float64))[:, None]
    c = F.conv2d(x, torch.ones((1, 1, n, n), dtype=torch.float64), padding=n // 2)[:, 0].numpy()
    assert (c == np.rint(c)).all()
    return np.rint(c).astype(np.int64)


def frame_hist(truth, pred, thresholds, scale, scales):
    """(frames, H, W) fields -> int64 (frames, nthr, S): per frame the bincount of c_f + (n^2 + 1) * o"""
    truth, pred = np.asarray(truth), np.asarray(pred)
    offs, S = layout(scales)
    out = np.zeros((truth.shape[0], len(thresholds), S), dtype=np.int64)
    for k, thr in enumerate(thresholds):
        o, f = events(truth, thr, scale), events(pred, thr, scale)
        for (a0, _), n in zip(offs, scales):
            idx = window_counts(f, n) + (n * n + 1) * o
            for i in range(truth.shape[0]):
                out[i, k, a0:a0 + 2 * (n * n + 1)] = np.bincount(idx[i].ravel(), minlength=2 * (n * n + 1))
    return out


def table(truth, pred, thresholds, scale, scales, T):
    """-> int64 (T, nthr, S): frame f belongs to row f mod T"""
    h = frame_hist(truth, pred, thresholds, scale, scales)
    out = np.zeros((T,) + h.shape[1:], dtype=np.int64)
    for i in range(h.shape[0]):
        out[i % T] += h[i]
    return out


def prob(field, thresholds, scale, n):
    """(frames, H, W) -> float32 (K, frames, H, W): np.float32(c) / np.float32(n * n)"""
    return np.stack([window_counts(events(field, thr, scale), n).astype(np.float32) / np.float32(n * n) for thr in thresholds])


def pixel_scores(truth, pred, thr, scale, n, bins=10):
    """the scores of one threshold and scale from the pixels themselves: the forecast p = c / n^2 and the observation o per pixel"""
    o = events(np.asarray(truth), thr, scale).ravel()
    c = window_counts(events(np.asarray(pred), thr, scale), n).ravel()
    p, of = c / float(n * n), o.astype(np.float64)
    total = o.size
    nan = float("nan")
    base = of.sum() / total
    brier = ((p - of) ** 2).sum() / total
    rel = res = 0.0
    for v in np.unique(c):                      # Murphy: over the distinct forecast values that occur
        m = c == v
        obar = of[m].mean()
        rel += m.sum() * (v / float(n * n) - obar) ** 2
        res += m.sum() * (obar - base) ** 2
    unc = base * (1.0 - base)
    pod, pofd = [], []
    for cstar in range(n * n + 1):              # warn when c >= c*
        warn = c >= cstar
        pod.append((warn & o).sum() / o.sum() if o.sum() else nan)
        pofd.append((warn & ~o).sum() / (~o).sum() if (~o).sum() else nan)
    pod, pofd = np.array(pod + [0.0]), np.array(pofd + [0.0])
    order = np.lexsort((pod, pofd))             # the trapezoid on ascending pofd (and pod, where a pofd repeats)
    x, y = pofd[order], pod[order]
    area = float((np.diff(x) * (y[1:] + y[:-1]) / 2.0).sum())
    count, mean, freq = [], [], []
    for b in range(bins):                       # b / bins <= p < (b + 1) / bins in integers, the last bin closed on the right
        m = (c * bins >= b * n * n) & ((c * bins < (b + 1) * n * n) | (b == bins - 1))
        count.append(int(m.sum()))
        mean.append(p[m].mean() if m.any() else nan)
        freq.append(of[m].mean() if m.any() else nan)
    return {"base_rate": base, "brier": brier, "reliability": rel / total, "resolution": res / total, "uncertainty": unc,
            "brier_skill": 1.0 - brier / unc if unc else nan, "pod": pod, "pofd": pofd, "roc_area": area,
            "count": np.array(count), "forecast_mean": np.array(mean), "observed_frequency": np.array(freq)}


def sparse_fields(frames, H, W, seed, plant=True):
    """joint_ref's radar-like pair: about 90 % exact zeros, smooth blobs, a weaker shifted forecast, NaN / +-Inf / negatives / > 1 planted"""
    return J.sparse_fields(frames, H, W, seed, plant)


def noise_fields(frames, H, W, seed, density, level=0.5):
    """two independent fields: `density` of the pixels at uniform values above `level`, the others 0"""
    rng = np.random.default_rng(seed)
    return tuple(np.where(rng.random((frames, H, W)) < density, rng.uniform(level, 1.0, (frames, H, W)), 0.0).astype(np.float32) for _ in range(2))


def _self_check():
    from scipy.ndimage import uniform_filter
    rng = np.random.default_rng(3)
    mask = rng.random((2, 9, 14)) < 0.4
    for n in (1, 3, 5, 33):
        want = np.stack([np.rint(uniform_filter(m.astype(np.float64), size=n, mode="constant", cval=0.0) * n * n) for m in mask]).astype(np.int64)
        assert (window_counts(mask, n) == want).all(), f"conv2d and uniform_filter disagree at n = {n}"
    t, p = sparse_fields(3, 9, 14, 5)
    h = frame_hist(t, p, [20.0, 40.0], 90.0, (1, 3))
    assert h.shape == (3, 2, 4 + 20) and (h[:, :, :4].sum(-1) == 9 * 14).all() and (h[:, :, 4:].sum(-1) == 9 * 14).all()


_self_check()
