"""The CPU yardstick of the track scores (csrc/tracks.hip; validate.track_entries), written differently from the kernel: the fields are
quantised with numpy in float32 (objects_ref.quantise), the event volume of a sample is labelled by scipy.ndimage.label with the full 3 x 3 x 3
structure, first and last frames come from scipy.ndimage.find_objects, volumes from np.bincount, canonical labels from scipy.ndimage.minimum of the
flat index, matching from scipy.ndimage.maximum of the other field's mask, and the entries from plain Python sums.  No union-find, no bit
planes, no frame-by-frame merging."""
import numpy as np
from scipy import ndimage

from objects_ref import events

FULL = ndimage.generate_binary_structure(3, 3)   # 26-connectivity


def cols(T):
    return 7 + 4 * T


def components(mask, other=None):
    """(T, H, W) bool -> (scipy's labels, per track: volume, t0, t1, canonical label 1 + first flat index, matched against `other`)"""
    lab, n = ndimage.label(mask, structure=FULL)
    ids = np.arange(1, n + 1)
    if n == 0:
        z = np.zeros(0, dtype=np.int64)
        return lab, z, z, z, z, np.zeros(0, dtype=bool)
    vol = np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int64)
    boxes = ndimage.find_objects(lab)
    t0 = np.array([b[0].start for b in boxes], dtype=np.int64)
    t1 = np.array([b[0].stop - 1 for b in boxes], dtype=np.int64)
    flat = np.arange(mask.size).reshape(mask.shape)
    first = np.asarray(ndimage.minimum(flat, labels=lab, index=ids), dtype=np.int64).reshape(-1)
    if other is None:
        matched = np.zeros(n, dtype=bool)
    else:
        matched = np.asarray(ndimage.maximum(other.astype(np.int64), labels=lab, index=ids)).reshape(-1) > 0
    return lab, vol, t0, t1, first + 1, matched


def canonical(mask, min_volume=1):
    """(T, H, W) bool -> int32 label volume: 1 + the flat index of the track's first voxel; 0 for the background and for tracks of fewer than
    min_volume voxels"""
    lab, vol, _, _, canon, _ = components(mask)
    table = np.zeros(len(vol) + 1, dtype=np.int64)
    table[1:] = np.where(vol >= min_volume, canon, 0)
    return table[lab].astype(np.int32)


def label_field(field, thr, scale, min_volume=1):
    """(..., T, H, W) float field -> int32 canonical labels of every volume"""
    field = np.asarray(field, dtype=np.float32)
    T, H, W = field.shape[-3:]
    out = np.stack([canonical(events(v, thr, scale), min_volume) for v in field.reshape(-1, T, H, W)])
    return out.reshape(field.shape)


def row(mask, other, min_volume=1):
    """the 7 + 4 T entries of one sample of one field: `mask` its event volume, `other` the other field's"""
    T = mask.shape[0]
    _, vol, t0, t1, _, matched = components(mask, other)
    out = [0] * cols(T)
    for v, a, b, m in zip(vol.tolist(), t0.tolist(), t1.tolist(), matched.tolist()):
        if v < min_volume:
            continue
        d = b - a + 1
        out[0] += 1
        out[1] += v
        out[2] += v * v
        out[3] += d
        if m:
            out[4] += 1
            out[5] += v
        if a == 0 and b == T - 1:
            out[6] += 1
        out[7 + a] += 1
        out[7 + T + b] += 1
        if a == 0:
            out[7 + 2 * T + b] += 1
        out[7 + 3 * T + d - 1] += 1
    return np.array(out, dtype=np.int64)


def sample_stats(target, pred, thresholds, scale, min_volume=1):
    """(B, T, H, W) fields -> (B, 2, nthr, 7 + 4 T) int64: field 0 = target, 1 = forecast"""
    target, pred = np.asarray(target, dtype=np.float32), np.asarray(pred, dtype=np.float32)
    B, T = target.shape[:2]
    out = np.zeros((B, 2, len(thresholds), cols(T)), dtype=np.int64)
    for b in range(B):
        for k, thr in enumerate(thresholds):
            o, p = events(target[b], thr, scale), events(pred[b], thr, scale)
            out[b, 0, k], out[b, 1, k] = row(o, p, min_volume), row(p, o, min_volume)
    return out


def table(target, pred, thresholds, scale, min_volume=1):
    """(B, T, H, W) fields -> (2, nthr, 7 + 4 T) int64, summed over the samples"""
    return sample_stats(target, pred, thresholds, scale, min_volume).sum(axis=0)


def identities(r, T):
    """the identities built into a row (or a sum of rows) of 7 + 4 T entries"""
    births, deaths, deaths0, hist = (r[7 + i * T:7 + (i + 1) * T] for i in range(4))
    return (births.sum() == deaths.sum() == hist.sum() == r[0] and deaths0.sum() == births[0] and deaths0[T - 1] == r[6]
            and r[3] == sum((k + 1) * int(h) for k, h in enumerate(hist)))


# ---- patterns: float32 (T, H, W) volumes whose events at any threshold in (0, scale] are the pattern
def mover(T, H, W, dy, dx, step=1):
    """one voxel per frame, starting where the walk stays inside, moving (dy, dx) * step per frame"""
    m = np.zeros((T, H, W), dtype=np.float32)
    y0 = 0 if dy >= 0 else H - 1
    x0 = 0 if dx >= 0 else W - 1
    for t in range(T):
        m[t, y0 + t * dy * step, x0 + t * dx * step] = 1
    return m


def serpentine3(T, H, W):
    """a one-voxel-wide path through rows and frames: in every frame every even row, joined to the next at alternating ends; the last row used of a
    frame continues in the next frame, which is walked the other way.  One track."""
    m = np.zeros((T, H, W), dtype=np.float32)
    rows = list(range(0, H, 2))
    for t in range(T):
        m[t, rows] = 1
        for i, y in enumerate(rows[:-1]):
            m[t, y + 1, W - 1 if i % 2 == 0 else 0] = 1
    return m


def spiral3(T, n):
    """objects_ref.spiral in every other frame, the frames between holding only the corner voxel that joins one spiral's outer end to the next
    one's: long union chains inside the frames, thin links between them.  One track."""
    from objects_ref import spiral
    s = spiral(n)
    m = np.zeros((T, n, n), dtype=np.float32)
    m[0::2] = s
    m[1::2, 0, 0] = 1
    return m


def lattice3(T, H, W):
    m = np.zeros((T, H, W), dtype=np.float32)
    m[0::2, 0::2, 0::2] = 1
    return m


def noise3(T, H, W, density, seed):
    return (np.random.default_rng(seed).random((T, H, W)) < density).astype(np.float32)


def fork(T, H, W):
    """a Y in time: two cells (columns 1 and W - 2) that approach one column per frame and merge, and the same mirrored in time further down (one
    cell that splits).  Two tracks, rows 1 and H - 2."""
    m = np.zeros((T, H, W), dtype=np.float32)
    mid = W // 2
    for t in range(T):
        a, b = min(1 + t, mid), max(W - 2 - t, mid)
        m[t, 1, a] = m[t, 1, b] = 1
        m[T - 1 - t, H - 2, a] = m[T - 1 - t, H - 2, b] = 1
    return m


def discs(B, T, H, W, seed, plant=False):
    """moving discs with random birth, life, radius, value and speed up to 1.5 px per frame on a zero background, values in [0.2, 1.0]; plant: NaN,
    +-Inf, negatives and values > 1 on top"""
    rng = np.random.default_rng(seed)
    f = np.zeros((B, T, H, W), dtype=np.float32)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for b in range(B):
        for _ in range(max(2, H * W // 160)):
            t0, life = int(rng.integers(0, T)), int(rng.integers(1, T + 1))
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.6, max(1.0, min(H, W) / 8))
            vy, vx = rng.uniform(-1.5, 1.5, 2)
            val = rng.uniform(0.2, 1.0)
            for t in range(t0, min(T, t0 + life)):
                inside = (yy - cy - vy * (t - t0)) ** 2 + (xx - cx - vx * (t - t0)) ** 2 <= r * r
                f[b, t][inside] = np.maximum(f[b, t][inside], np.float32(val))
    if plant:
        flat = f.reshape(-1)
        for k, bad in enumerate((np.nan, np.inf, -np.inf, -0.25, 1.75, np.nan, 1.0, np.inf)):
            flat[(k * 7919 + seed) % flat.size] = bad
    return f


def _self_check():
    """scipy's components against a plain flood fill on a random volume, and the canonical labels against the definition"""
    m = noise3(4, 5, 6, 0.12, 3) > 0
    want = np.zeros(m.shape, dtype=np.int32)
    for start in zip(*np.nonzero(m)):
        if want[start]:
            continue
        stack, name = [start], (start[0] * m.shape[1] + start[1]) * m.shape[2] + start[2] + 1
        want[start] = name
        while stack:
            t, y, x = stack.pop()
            for nt in range(max(t - 1, 0), min(t + 2, m.shape[0])):
                for ny in range(max(y - 1, 0), min(y + 2, m.shape[1])):
                    for nx in range(max(x - 1, 0), min(x + 2, m.shape[2])):
                        if m[nt, ny, nx] and not want[nt, ny, nx]:
                            want[nt, ny, nx] = name
                            stack.append((nt, ny, nx))
    assert (canonical(m) == want).all(), "scipy's labels, made canonical, are not the flood fill's"


_self_check()
