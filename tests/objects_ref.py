"""The CPU yardstick of the object scores (csrc/objects.hip; validate.object_entries), written differently from the kernel: the fields are
quantised with numpy in float32 (NaN put to 0 first, as fmaxf does), the event mask is labelled by scipy.ndimage.label with a full 3 x 3
structure, areas come from np.bincount, canonical labels from scipy.ndimage.minimum of the flat index, matching from a boolean mask and the
log2 bin from np.frexp.  No union-find, no bit fields, no runs."""
import numpy as np
from scipy import ndimage

COLS, BINS = 23, 17
EIGHT = np.ones((3, 3), dtype=np.int64)


def quantise(v, scale):
    """fp32 field -> float32 levels: floor(clip(v, 0, 1) * scale) in float32; NaN -> 0 (fmaxf(NaN, 0) = 0)"""
    v = np.asarray(v, dtype=np.float32)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.floor(np.clip(v, np.float32(0), np.float32(1)) * np.float32(scale))


def events(v, thr, scale):
    return quantise(v, scale) >= np.float32(thr)


def components(mask):
    """(H, W) bool -> (scipy's label image, the objects' ids 1 .. n, their areas, their canonical labels 1 + first row-major index)"""
    lab, n = ndimage.label(mask, structure=EIGHT)
    ids = np.arange(1, n + 1)
    areas = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    flat = np.arange(mask.size).reshape(mask.shape)
    first = np.asarray(ndimage.minimum(flat, labels=lab, index=ids), dtype=np.int64).reshape(-1) if n else np.zeros(0, dtype=np.int64)
    return lab, ids, areas.astype(np.int64), first + 1


def canonical(mask, min_area=1):
    """(H, W) bool -> int32 label image: 1 + the row-major index of the object's first pixel; 0 for the background and for objects of
    fewer than min_area pixels"""
    lab, ids, areas, canon = components(mask)
    table = np.zeros(len(ids) + 1, dtype=np.int64)
    table[1:] = np.where(areas >= min_area, canon, 0)
    return table[lab].astype(np.int32)


def label_field(field, thr, scale, min_area=1):
    """(..., H, W) float field -> int32 canonical labels of every frame"""
    field = np.asarray(field, dtype=np.float32)
    H, W = field.shape[-2:]
    out = np.stack([canonical(events(fr, thr, scale), min_area) for fr in field.reshape(-1, H, W)]) if field.size else np.zeros((0, H, W), np.int32)
    return out.reshape(field.shape)


def log2_bin(area):
    """floor(log2(area)) of positive integers from the binary exponent: area = m * 2^e with 0.5 <= m < 1, so the bin is e - 1"""
    return np.frexp(np.asarray(area, dtype=np.float64))[1] - 1


def row(mask, other, min_area=1):
    """the 23 entries of one frame of one field: `mask` its events, `other` the other field's"""
    lab, ids, areas, _ = components(mask)
    keep = areas >= min_area
    touched = np.zeros(len(ids) + 1, dtype=bool)
    touched[np.unique(lab[other & mask])] = True
    matched = touched[1:] & keep
    a = areas[keep]
    out = np.zeros(COLS, dtype=np.int64)
    out[0], out[1], out[2], out[3] = a.size, a.sum(), (a * a).sum(), a.max() if a.size else 0
    out[4], out[5] = matched.sum(), areas[matched].sum()
    out[6:] = np.bincount(log2_bin(a), minlength=BINS) if a.size else 0
    return out


def frame_stats(target, pred, thresholds, scale, min_area=1):
    """(frames, H, W) fields -> (frames, 2, nthr, 23) int64: field 0 = target, 1 = forecast"""
    target, pred = np.asarray(target, dtype=np.float32), np.asarray(pred, dtype=np.float32)
    out = np.zeros((target.shape[0], 2, len(thresholds), COLS), dtype=np.int64)
    for f in range(target.shape[0]):
        for k, thr in enumerate(thresholds):
            o, p = events(target[f], thr, scale), events(pred[f], thr, scale)
            out[f, 0, k], out[f, 1, k] = row(o, p, min_area), row(p, o, min_area)
    return out


def table(target, pred, thresholds, scale, T, min_area=1):
    """(frames, H, W) fields -> (T, 2, nthr, 23) int64: frame f belongs to row f mod T"""
    st = frame_stats(target, pred, thresholds, scale, min_area)
    out = np.zeros((T,) + st.shape[1:], dtype=np.int64)
    for f in range(st.shape[0]):
        out[f % T] += st[f]
    return out


# ---- patterns: float32 (H, W) fields whose events at any threshold in (0, scale] are the pattern
def serpentine(H, W):
    """a one-pixel-wide path: every even row full, joined to the next at alternating ends.  One object."""
    m = np.zeros((H, W), dtype=np.float32)
    m[0::2] = 1
    for i, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            m[y, W - 1 if i % 2 == 0 else 0] = 1
    return m


def spiral(n):
    """a one-pixel-wide square spiral with one-pixel gaps, walked inwards from (0, 0).  One object."""
    m = np.zeros((n, n), dtype=np.float32)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    while True:
        moved = 0
        while True:
            ny, nx = y + dy, x + dx
            ahead = (ny + dy, nx + dx)
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx]:
                break
            if 0 <= ahead[0] < n and 0 <= ahead[1] < n and m[ahead]:
                break
            y, x = ny, nx
            m[y, x] = 1
            moved += 1
        if moved < 2:
            return m
        dy, dx = dx, -dy


def comb(H, W):
    """vertical teeth on every other column that meet only in the last row: one object, merged late"""
    m = np.zeros((H, W), dtype=np.float32)
    m[:, 0::2] = 1
    m[H - 1] = 1
    return m


def lattice(H, W):
    """isolated pixels on a stride-2 lattice: ceil(H / 2) * ceil(W / 2) objects of one pixel"""
    m = np.zeros((H, W), dtype=np.float32)
    m[0::2, 0::2] = 1
    return m


def checkerboard(H, W):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return ((y + x) % 2 == 0).astype(np.float32)


def noise(H, W, density, seed):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.float32)


def radar(frames, H, W, seed, plant=False):
    """about 90 % zeros plus smoothed blobs with ragged edges, values in [0, 1.3); plant: NaN, +-Inf, negatives and values > 1 on top"""
    rng = np.random.default_rng(seed)
    raw = ndimage.gaussian_filter(rng.random((frames, H, W)), (0, max(H, W) / 24 + 0.5, max(H, W) / 24 + 0.5), mode="constant")
    raw = raw + 0.15 * raw.std() * rng.standard_normal(raw.shape)
    cut = np.quantile(raw, 0.9)
    fld = np.where(raw < cut, 0.0, 0.25 + (raw - cut) / (raw.max() - cut + 1e-12)).astype(np.float32)
    if plant:
        flat = fld.reshape(-1)
        for k, bad in enumerate((np.nan, np.inf, -np.inf, -0.25, 1.75, np.nan, 1.0, np.inf)):
            flat[(k * 7919 + seed) % flat.size] = bad
    return fld


def _self_check():
    """scipy's components against a plain flood fill on a random mask, and the canonical labels against the definition"""
    m = noise(9, 11, 0.45, 3) > 0
    want = np.zeros(m.shape, dtype=np.int32)
    for start in zip(*np.nonzero(m)):
        if want[start]:
            continue
        stack, name = [start], start[0] * m.shape[1] + start[1] + 1   # row-major order: the first pixel met is the smallest index
        want[start] = name
        while stack:
            y, x = stack.pop()
            for ny in range(max(y - 1, 0), min(y + 2, m.shape[0])):
                for nx in range(max(x - 1, 0), min(x + 2, m.shape[1])):
                    if m[ny, nx] and not want[ny, nx]:
                        want[ny, nx] = name
                        stack.append((ny, nx))
    assert (canonical(m) == want).all(), "scipy's labels, made canonical, are not the flood fill's"
    assert log2_bin([1, 2, 3, 4, 7, 8, 65535, 65536]).tolist() == [0, 1, 1, 2, 2, 3, 15, 16]


_self_check()
