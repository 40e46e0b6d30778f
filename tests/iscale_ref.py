"""The CPU yardstick of the intensity-scale skill score (csrc/neighbour.hip: adnm_valid_iscale_accum; validate.intensity_scale_entries), written
differently from the kernel: the fields quantised in numpy float32 the way adnm_eval_counts quantises them (verify_ref.quant), thresholded, zero
padded to the P x P domain, and
  ref_sums    the block sums by reshape(P/s, s, P/s, s).sum((1, 3)) in int64: A = sum o^2, F = sum f^2, C = sum o f per level and threshold;
  components  from those sums, in Python integers and one division: E_j - E_(j+1);
  haar_bands  independently, the same components from an explicit orthonormal Haar matrix (recursive Kronecker), C = H Z H^T, with the band
              energies picked by a mask of the coefficient's scale.
Sums are integers: every comparison of the kernel against ref_sums is exact.  The reference project has no such score, so nothing here is
recorded from it."""
import numpy as np

import verify_ref as R

THR, SCALE = R.THR, R.SCALE
THR_SETS = {"one": [30], "default": THR, "five": [5, 20, 30, 35, 40], "eight": R.THR_SETS["eight"]}


def levels(H, W):
    """-> (P, L): the smallest power of two >= max(H, W) and its log2"""
    L = 0
    while (1 << L) < max(H, W):
        L += 1
    return 1 << L, L


def padded_events(field, thr, scale, dtype=np.int64):
    """(frames, H, W) floats -> (frames, P, P) of 0 / 1: the event q >= thr on the quantised field, zeros outside the frame"""
    q = R.quant(np.asarray(field), scale)
    n, H, W = q.shape
    P, _ = levels(H, W)
    out = np.zeros((n, P, P), dtype=dtype)
    out[:, :H, :W] = q >= np.float32(thr)
    return out


def block_counts(z, s):
    """(frames, P, P) -> int64 (frames, P/s, P/s): the sums over the s x s blocks that tile the domain from its origin"""
    n, P, _ = z.shape
    return z.reshape(n, P // s, s, P // s, s).sum(axis=(2, 4), dtype=np.int64)


def ref_sums(truth, pred, thresholds, scale):
    """truth, pred: (frames, H, W) float arrays -> int64 (frames, L + 1, 3 * nthr): A, F, C per level and threshold"""
    truth, pred = np.asarray(truth), np.asarray(pred)
    n, H, W = truth.shape
    _, L = levels(H, W)
    out = np.zeros((n, L + 1, 3 * len(thresholds)), dtype=np.int64)
    for k, thr in enumerate(thresholds):
        zo, zf = padded_events(truth, thr, scale, np.uint8), padded_events(pred, thr, scale, np.uint8)   # (bytes: a 1024 x 1024 domain stays small)
        for l in range(L + 1):
            o, f = block_counts(zo, 1 << l), block_counts(zf, 1 << l)
            out[:, l, 3 * k + 0] = (o * o).sum(axis=(1, 2))
            out[:, l, 3 * k + 1] = (f * f).sum(axis=(1, 2))
            out[:, l, 3 * k + 2] = (o * f).sum(axis=(1, 2))
    return out


def components(x, frames, P):
    """(L + 1,) integer sums X_l over `frames` frames -> (L + 1,) float64: E_j - E_(j+1) for j < L, E_L for the last, E_l = X_l / (4^l frames P^2),
    formed with the numerator 4 X_j - X_(j+1) in Python integers"""
    x = [int(v) for v in x]
    L = len(x) - 1
    return np.array([(4 * x[j] - (x[j + 1] if j < L else 0)) / (4 ** (j + 1) * frames * P * P) for j in range(L + 1)], dtype=np.float64)


def haar_matrix(P):
    """-> (the orthonormal P x P Haar matrix by the recursive Kronecker construction, the level of each of its rows: row 0 is the mean, level
    L = log2 P; a row of level j < L is a difference of two neighbouring blocks of 2^j samples)"""
    h, lev = np.ones((1, 1)), [0]
    while h.shape[0] < P:
        n = h.shape[0]
        h = np.concatenate([np.kron(h, [1.0, 1.0]), np.kron(np.eye(n), [1.0, -1.0])]) / np.sqrt(2.0)
        lev = [v + 1 for v in lev] + [0] * n
    assert np.abs(h @ h.T - np.eye(P)).max() < 1e-12
    return h, np.array(lev)


def haar_bands(z):
    """z: (P, P) field -> (L + 1,) float64: the mean over the domain of the squared Haar component of scale 2^j, j = 0 .. L (the last: the
    squared domain mean).  A row of level >= j is constant on blocks of 2^j samples, so the coefficients with min(level r, level c) >= j span
    the fields that are constant on 2^j x 2^j blocks: the band of scale 2^j is the mask min(level r, level c) == j."""
    P = z.shape[0]
    h, lev = haar_matrix(P)
    L = int(lev[0])
    c = h @ np.asarray(z, dtype=np.float64) @ h.T
    band = np.minimum(lev[:, None], lev[None, :])
    return np.array([(c * c)[band == j].sum() for j in range(L + 1)]) / float(P * P)


def nonstandard_bands(z):
    """the same bands the way the score is defined (Casati 2004): the 2-D discrete Haar transform by levels (the NON-standard decomposition: at
    each level the three detail images of the 2 x 2 averaging step), from an explicit orthonormal matrix per level"""
    z = np.asarray(z, dtype=np.float64)
    P = z.shape[0]
    out = []
    a = z
    while a.shape[0] > 1:
        n = a.shape[0] // 2
        lo, hi = np.kron(np.eye(n), [1.0, 1.0]) / np.sqrt(2.0), np.kron(np.eye(n), [1.0, -1.0]) / np.sqrt(2.0)
        out.append(((lo @ a @ hi.T) ** 2).sum() + ((hi @ a @ lo.T) ** 2).sum() + ((hi @ a @ hi.T) ** 2).sum())
        a = lo @ a @ lo.T
    out.append((a ** 2).sum())
    return np.array(out) / float(P * P)


def entries(sums, frames, shape, thresholds):
    """(L + 1, 3 * nthr) integer sums over `frames` frames -> {thr: {...}}: the definitions of the score, written out one threshold at a time"""
    P, L = levels(*shape)
    N = float(frames * P * P)
    res = {}
    for k, thr in enumerate(thresholds):
        a, f, c = (np.asarray(sums)[:, 3 * k + i] for i in range(3))
        d = a + f - 2 * c
        mse, en_o, en_f = components(d, frames, P), components(a, frames, P), components(f, frames, P)
        with np.errstate(divide="ignore", invalid="ignore"):
            eps, bias = a[0] / N, np.float64(f[0]) / np.float64(a[0])
            rand = bias * eps * (1 - eps) + eps * (1 - bias * eps)
            res[thr] = {"mse": mse, "mse_total": d[0] / N, "base_rate": eps, "bias": bias, "mse_random": rand, "skill": 1 - mse * (L + 1) / rand,
                        "energy_target": en_o, "energy_forecast": en_f, "energy_rel_diff": (en_f - en_o) / (en_f + en_o), "mse_share": mse / (d[0] / N)}
    return res


# ------------------------------------------------------------------------------------------------ the routes against one another
ROUTE_CASES = [(1, 1), (1, 7), (5, 7), (8, 8), (13, 32), (33, 20), (64, 64)]   # (H, W); a field has at most 2^12 pixels, far below the 2^16 of the bar


def route_report():
    """-> (lines, the largest deviation): for every case and threshold the components of the binary error, of the target and of the forecast by
    the three routes (block sums; H Z H^T with the band mask; the transform by levels), frame by frame, and the largest absolute difference
    between the block-sum route and each of the others.  Every component is a sum of at most P^2 <= 2^16 squares of magnitude <= 1 divided
    by P^2: 1e-10 is far above what double rounding can add up to, far below any wrong band (>= 1 / P^2 / 4^L)."""
    lines, worst = [], 0.0
    for H, W in ROUTE_CASES:
        P, L = levels(H, W)
        t, p = radar_fields(3, H, W, H + W, plant=H * W > 8)
        sums = ref_sums(t, p, THR, SCALE)
        dev = [0.0, 0.0]
        for k, thr in enumerate(THR):
            zo, zf = padded_events(t, thr, SCALE), padded_events(p, thr, SCALE)
            for n in range(len(t)):
                a, f, c = (sums[n, :, 3 * k + i] for i in range(3))
                for x, z in ((a + f - 2 * c, zf[n] - zo[n]), (a, zo[n]), (f, zf[n])):
                    mine = components(x, 1, P)
                    for i, other in enumerate((haar_bands(z), nonstandard_bands(z))):
                        dev[i] = max(dev[i], float(np.abs(mine - other).max()))
        lines.append(f"  {H:3d} x {W:3d}  P {P:3d}  L {L}: H Z H^T {dev[0]:.3e}   by levels {dev[1]:.3e}")
        worst = max(worst, *dev)
    return lines, worst


# ------------------------------------------------------------------------------------------------ patterns
def radar_fields(frames, H, W, seed, plant=False):
    """verify_ref.radar_fields; plant: NaN, +Inf, -Inf, negatives and values > 1 at random places and at the frame's corners, in both fields"""
    t, p = R.radar_fields(frames, H, W, seed)
    if plant:
        rng = np.random.default_rng(seed + 100)
        for a in (t, p):
            for value in (np.nan, np.inf, -np.inf, -0.5, 1.5):
                a.reshape(-1)[rng.choice(a.size, max(1, a.size // 50), replace=False)] = value
        t[0, 0, 0], p[0, -1, -1], t[-1, -1, 0], p[-1, 0, -1] = np.inf, np.inf, np.nan, 1.5
    return t, p


def noise(frames, H, W, density, seed):
    """-> (target, forecast): independent fields with an event (0.9) at `density` of the pixels"""
    rng = np.random.default_rng(seed)
    return tuple(np.where(rng.random((frames, H, W)) < density, 0.9, 0.0).astype(np.float32) for _ in range(2))


def checkerboard(frames, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.broadcast_to(np.where((yy + xx) % 2 == 0, 0.9, 0.0).astype(np.float32), (frames, H, W)).copy()


def half_plane(frames, H, W):
    out = np.zeros((frames, H, W), dtype=np.float32)
    out[:, :, :(W + 1) // 2] = 0.9
    return out


def shifted(field, px):
    """the field moved px pixels along x, zeros entering"""
    out = np.zeros_like(field)
    if px < field.shape[-1]:
        out[..., px:] = field[..., :field.shape[-1] - px]
    return out


if __name__ == "__main__":
    import os
    body, top = route_report()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "iscale_error.txt"), "w") as out:
        out.write("intensity-scale components: the block-sum form against the orthonormal 2-D Haar transform on the CPU yardstick (tests/iscale_ref.py;\n"
                  "value_scale 90, thresholds 20 30 35 40, 3 frames a case): the largest absolute deviation of a component of the error, of the target and\n"
                  "of the forecast.  The bar of tests/test_iscale_host.py is 1e-10.\n\n" + "\n".join(body) + f"\n\nlargest deviation {top:.3e}\n")
    print("\n".join(body), f"\nlargest deviation {top:.3e}")
