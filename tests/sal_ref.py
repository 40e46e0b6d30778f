"""The CPU yardstick of the per-object intensity moments and the SAL scores (csrc/sal.hip; validate.sal_entries), written differently from the
kernel: the fields are quantised with numpy (objects_ref.quantise), the event mask is labelled by scipy.ndimage.label with a full 3 x 3
structure, the weights are summed per label by scipy.ndimage.sum and their maximum taken by scipy.ndimage.maximum, the moments become Python
integers and the scores are formed in float64 object by object.  No union-find, no bit fields, no runs, no records."""
import math

import numpy as np
from scipy import ndimage

import objects_ref as O
from objects_ref import checkerboard, comb, lattice, noise, radar, serpentine, spiral  # noqa: F401  (the generators, for the tests)

COLS = 12


def weights(field, scale, intensity=None):
    """(H, W) float field -> int64 weights w = intensity[q] (q itself for None)"""
    q = O.quantise(field, scale).astype(np.int64)
    return q if intensity is None else np.asarray(intensity, dtype=np.int64)[q]


def mass(w):
    """(H, W) int64 weights -> Python integers (M, Mx, My), x = column and y = row"""
    y, x = np.meshgrid(np.arange(w.shape[0], dtype=np.int64), np.arange(w.shape[1], dtype=np.int64), indexing="ij")
    return int(w.sum()), int((w * x).sum()), int((w * y).sum())


def objects(field, thr, scale, min_area=1, intensity=None):
    """(H, W) float field -> [(first row-major index, area, R, Q, X, Y)] of the objects of at least min_area pixels, Python integers"""
    mask = O.events(field, thr, scale)
    lab, ids, areas, canon = O.components(mask)
    if not len(ids):
        return []
    w = weights(field, scale, intensity)
    y, x = np.meshgrid(np.arange(w.shape[0], dtype=np.int64), np.arange(w.shape[1], dtype=np.int64), indexing="ij")
    # scipy sums in float64: every partial sum is an integer below 2^53, so the sums are exact
    R, X, Y = (np.rint(np.atleast_1d(ndimage.sum(a, labels=lab, index=ids))).astype(np.int64) for a in (w, w * x, w * y))
    Q = np.atleast_1d(ndimage.maximum(w, labels=lab, index=ids)).astype(np.int64)
    return [(int(canon[i]) - 1, int(areas[i]), int(R[i]), int(Q[i]), int(X[i]), int(Y[i])) for i in range(len(ids)) if areas[i] >= min_area]


def moments(field, thr, scale, min_area=1, intensity=None):
    """(..., H, W) float field -> int64 (..., 4, H, W): R, Q, X, Y at the first pixel of every kept object, 0 elsewhere"""
    field = np.asarray(field, dtype=np.float32)
    H, W = field.shape[-2:]
    frames = field.reshape(-1, H, W)
    out = np.zeros((frames.shape[0], 4, H * W), dtype=np.int64)
    for f, fr in enumerate(frames):
        for first, _, R, Q, X, Y in objects(fr, thr, scale, min_area, intensity):
            out[f, :, first] = (R, Q, X, Y)
    return out.reshape(field.shape[:-2] + (4, H, W))


def structure(field, thr, scale, min_area=1, intensity=None):
    """(H, W) field -> (M, (cx, cy) or None, V, r, kept objects): the whole-field mass and centre, the scaled volume and the weighted mean
    distance of the objects' centroids from the centre (None without an object)"""
    M, Mx, My = mass(weights(field, scale, intensity))
    c = (Mx / M, My / M) if M > 0 else None
    kept = [(R, Q, X, Y) for _, _, R, Q, X, Y in objects(field, thr, scale, min_area, intensity) if R > 0]
    if not kept:
        return M, c, None, None, 0
    total = float(sum(R for R, _, _, _ in kept))
    V = math.fsum(R * (R / Q) for R, Q, _, _ in kept) / total
    r = math.fsum(R * math.hypot(X / R - c[0], Y / R - c[1]) for R, _, X, Y in kept) / total
    return M, c, V, r, len(kept)


def scores(target, pred, thr, scale, min_area=1, intensity=None):
    """one frame pair -> {"A", "L1", "S", "L2", "L"} (None where undefined), "only_target", "only_forecast" """
    H, W = target.shape
    d = math.hypot(H, W)
    Mo, co, Vo, ro, no = structure(target, thr, scale, min_area, intensity)
    Mf, cf, Vf, rf, nf = structure(pred, thr, scale, min_area, intensity)
    res = dict(A=None, L1=None, S=None, L2=None, L=None, only_target=bool(no and not nf), only_forecast=bool(nf and not no))
    if Mo + Mf > 0:
        res["A"] = (Mf - Mo) / (0.5 * (Mf + Mo))
    if Mo > 0 and Mf > 0:
        res["L1"] = math.hypot(cf[0] - co[0], cf[1] - co[1]) / d
    if no and nf:
        res["S"] = (Vf - Vo) / (0.5 * (Vf + Vo))
        res["L2"] = 2.0 * abs(rf - ro) / d
        res["L"] = res["L1"] + res["L2"]
    return res


def row(target, pred, thr, scale, min_area=1, intensity=None):
    """the 12 entries of one frame pair at one threshold"""
    s = scores(target, pred, thr, scale, min_area, intensity)
    out = np.zeros(COLS, dtype=np.float64)
    if s["A"] is not None:
        out[0:3] = (1.0, s["A"], abs(s["A"]))
    if s["L1"] is not None:
        out[3:5] = (1.0, s["L1"])
    if s["S"] is not None:
        out[5:10] = (1.0, s["S"], abs(s["S"]), s["L2"], s["L"])
    out[10], out[11] = float(s["only_target"]), float(s["only_forecast"])
    return out


def frame_rows(target, pred, thresholds, scale, min_area=1, intensity=None):
    """(frames, H, W) fields -> (frames, nthr, 12) float64"""
    target, pred = np.asarray(target, dtype=np.float32), np.asarray(pred, dtype=np.float32)
    return np.stack([np.stack([row(t, p, thr, scale, min_area, intensity) for thr in thresholds]) for t, p in zip(target, pred)])


def fold(rows, T, onto=None):
    """(frames, nthr, 12) rows -> (T, nthr, 12): per frame index the batch sum, samples ascending from 0.0, added once to `onto` — the order
    the device keeps, in numpy float64 adds"""
    out = np.zeros((T,) + rows.shape[1:], dtype=np.float64) if onto is None else np.array(onto, dtype=np.float64)
    for t in range(T):
        batch = np.zeros(rows.shape[1:], dtype=np.float64)
        for b in range(rows.shape[0] // T):
            batch = batch + rows[b * T + t]
        out[t] = out[t] + batch
    return out


def blobs(H, W, n=6, seed=0, margin=12, sigma=(2.0, 4.0)):
    """n Gaussian blobs of peak 0.35 .. 0.95 whose centres keep `margin` pixels from the border: float32 (H, W) in [0, 1)"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = np.zeros((H, W))
    for _ in range(n):
        cy, cx, s, a = rng.uniform(margin, H - margin), rng.uniform(margin, W - margin), rng.uniform(*sigma), rng.uniform(0.35, 0.95)
        f = np.maximum(f, a * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s)))
    return f.astype(np.float32)


def _self_check():
    """scipy's sums per label against plain loops over the pixels on a random field"""
    rng = np.random.default_rng(5)
    f = (rng.random((7, 9)) * (rng.random((7, 9)) < 0.5)).astype(np.float32)
    lab = O.canonical(O.events(f, 20, 90.0))
    q = O.quantise(f, 90.0).astype(int)
    want = {}
    for yy in range(7):
        for xx in range(9):
            if lab[yy, xx]:
                R, Q, X, Y, a = want.get(lab[yy, xx] - 1, (0, 0, 0, 0, 0))
                want[lab[yy, xx] - 1] = (R + q[yy, xx], max(Q, q[yy, xx]), X + q[yy, xx] * xx, Y + q[yy, xx] * yy, a + 1)
    got = {first: (R, Q, X, Y, area) for first, area, R, Q, X, Y in objects(f, 20, 90.0)}
    assert got == want and len(got) > 1, "scipy's sums by label are not the loops'"


_self_check()
