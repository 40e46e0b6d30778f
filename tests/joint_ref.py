"""The CPU yardstick of the joint intensity histogram (csrc/joint.hip; validate.joint_entries), written differently from both: the fields
are quantised with numpy in float32 (NaN put to 0 first, as fmaxf does), counted with np.histogram2d on integer edges per frame, and
every curve comes from boolean masks per threshold instead of cumulative sums.  The module checks itself once, when it is imported,
against np.bincount of the packed index."""
import numpy as np


def levels(scale):
    return int(np.floor(np.float32(scale))) + 1


def quantise(v, scale):
    """fp32 field -> int64 levels 0 .. L - 1: floor(clip(v, 0, 1) * scale) in float32; NaN -> 0 (fmaxf(NaN, 0) = 0)"""
    v = np.asarray(v, dtype=np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.floor(np.clip(v, np.float32(0), np.float32(1)) * np.float32(scale)).astype(np.int64)


def frame_hist(target, pred, scale):
    """(frames, ...) fields -> (frames, L, L) int64, [f][q_o][q_f], one np.histogram2d per frame"""
    L = levels(scale)
    edges = np.arange(L + 1) - 0.5
    o, f = quantise(target, scale), quantise(pred, scale)
    out = np.zeros((o.shape[0], L, L), dtype=np.int64)
    for i in range(o.shape[0]):
        h, _, _ = np.histogram2d(o[i].ravel(), f[i].ravel(), bins=(edges, edges))
        out[i] = np.rint(h).astype(np.int64)
    return out


def table(target, pred, scale, T):
    """(frames, ...) fields -> (T, L, L) int64: frame f belongs to row f mod T"""
    h = frame_hist(target, pred, scale)
    out = np.zeros((T,) + h.shape[1:], dtype=np.int64)
    for i in range(h.shape[0]):
        out[i % T] += h[i]
    return out


def pairs(hist):
    """(L, L) counts -> the level pairs (o, f) and their counts, the non-empty bins only"""
    o, f = np.nonzero(hist)
    return o, f, hist[o, f]


def counts_at(hist, v):
    """(L, L) counts -> TP, FN, FP, TN with the event q >= v, by masks over the bins"""
    o, f, n = pairs(np.asarray(hist))
    eo, ef = o >= v, f >= v
    return int(n[eo & ef].sum()), int(n[eo & ~ef].sum()), int(n[~eo & ef].sum()), int(n[~eo & ~ef].sum())


def curves(hist):
    """(L, L) counts -> {TP, FN, FP, TN: int64 (L,)} at every integer threshold"""
    L = hist.shape[-1]
    rows = np.array([counts_at(hist, v) for v in range(L)], dtype=np.int64)
    return {k: rows[:, i] for i, k in enumerate(("TP", "FN", "FP", "TN"))}


def qq(hist):
    """qq[v] = the smallest u with CDF_o(u) >= CDF_f(v), by a plain search on the counts"""
    L = hist.shape[-1]
    m_o, m_f = hist.sum(axis=1), hist.sum(axis=0)
    out = np.zeros(L, dtype=np.int64)
    for v in range(L):
        below = int(m_f[:v + 1].sum())
        u = 0
        while int(m_o[:u + 1].sum()) < below:
            u += 1
        out[v] = u
    return out


def moments(hist):
    """(L, L) counts -> (conditional mean per target level, Pearson's r, mean error) from the expanded sample, in float64"""
    o, f, n = pairs(np.asarray(hist))
    so, sf = np.repeat(o, n).astype(np.float64), np.repeat(f, n).astype(np.float64)
    L = hist.shape[-1]
    cond = np.array([sf[so == v].mean() if (so == v).any() else np.nan for v in range(L)])
    r = np.nan if so.size == 0 or so.std() == 0 or sf.std() == 0 else float(np.corrcoef(so, sf)[0, 1])
    return cond, r, float((sf - so).mean()) if so.size else np.nan


def sparse_fields(frames, H, W, seed, plant=True):
    """-> (target, forecast) float32 (frames, H, W): about 90 % exact zeros plus smooth blobs reaching past 1, the forecast a weaker,
    shifted copy with its own zeros; with `plant` a few NaN, +-Inf, negative and > 1 values in both (where the frame has room)"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = []
    for which in range(2):
        fld = np.zeros((frames, H, W))
        for i in range(frames):
            for _ in range(2):
                cy, cx, s = rng.uniform(0, H), rng.uniform(0, W) + 1.5 * which, rng.uniform(0.8, 0.12 * max(H, W) + 1.0)
                fld[i] += rng.uniform(0.3, 1.3) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
        fld = np.where(fld < np.quantile(fld, 0.9), 0.0, fld * (0.8 if which else 1.0)).astype(np.float32)
        if plant:
            flat = fld.reshape(-1)
            for k, bad in enumerate((np.nan, np.inf, -np.inf, -0.25, 1.75, np.nan, 1.0)):
                flat[(k * 7919 + 3 * which + seed) % flat.size] = bad
        out.append(fld)
    return out[0], out[1]


def uniform_fields(frames, H, W, seed):
    """two independent fields of uniform noise over slightly more than [0, 1]: every level of both"""
    rng = np.random.default_rng(seed)
    return tuple(rng.uniform(-0.02, 1.02, (frames, H, W)).astype(np.float32) for _ in range(2))


def _self_check():
    for scale in (90.0, 89.5, 1.0, 127.99):
        t, p = sparse_fields(3, 9, 14, 5)
        u = uniform_fields(3, 9, 14, 6)
        for a, b in ((t, p), u):
            L = levels(scale)
            o, f = quantise(a, scale), quantise(b, scale)
            assert o.min() >= 0 and f.min() >= 0 and o.max() <= L - 1 and f.max() <= L - 1
            want = np.stack([np.bincount((o[i] * L + f[i]).ravel(), minlength=L * L).reshape(L, L) for i in range(3)])
            assert (frame_hist(a, b, scale) == want).all(), "histogram2d and bincount disagree"
            assert (table(a, b, scale, 1)[0] == want.sum(0)).all()


_self_check()
