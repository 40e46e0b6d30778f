"""The CPU yardstick of the radially averaged power spectra (include/adnm_hip.h: adnm_valid_spectrum_accum), written differently from
the kernel: numpy.fft.fft2 of the float64 field, a bin IMAGE from np.rint(np.sqrt(...)) on np.fft.fftfreq, and sums by boolean mask per
bin.  No row packing, no symmetry, no integer bin rule.  Also a float32 restatement (scipy.fft.fft2 of float32 input computes in
complex64), which says how far an fp32 transform of these fields lies from the float64 one, and the test fields."""
import numpy as np

SCALE = 255.0
# (frames, H, W, sigma of the Gaussian smoothing, seed): the shapes of tests/test_spectrum_gpu.py, white noise and two smoothed fields
CASES = [(2, 8, 8, 0, 1), (2, 16, 64, 2, 2), (2, 64, 16, 2, 3), (3, 32, 32, 0, 4), (2, 128, 128, 6, 5), (2, 128, 128, 0, 6), (2, 512, 8, 2, 7), (1, 8, 512, 2, 8)]


def case_id(case):
    return "x".join(map(str, case[:3])) + f"-s{case[3]}"


def fields(n, H, W, sigma, seed):
    """-> (target, forecast), float32 (n, H, W): uniform noise, optionally smoothed periodically, stretched to [-0.1, 1.1] so that the
    clip cuts on both sides; the forecast is the target smoothed a little more plus its own noise (coherent at large scales only)"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)

    def stretch(a):
        lo, hi = a.min(axis=(1, 2), keepdims=True), a.max(axis=(1, 2), keepdims=True)
        return ((a - lo) / (hi - lo) * 1.2 - 0.1).astype(np.float32)

    def smooth(a, s):
        return np.stack([gaussian_filter(f, s, mode="wrap") for f in a]) if s > 0 else a

    base, own = rng.random((n, H, W)), rng.random((n, H, W))
    t = smooth(base, sigma)
    p = smooth(0.7 * base + 0.3 * own, sigma + 1 if sigma else 0)
    return stretch(t), stretch(p)


def clipped(a, scale, dtype=np.float64):
    """the field the spectrum is taken of: clip(a, 0, 1) * scale in float32 (a NaN stays a NaN), then `dtype`"""
    return (np.clip(np.asarray(a, dtype=np.float32), np.float32(0), np.float32(1)) * np.float32(scale)).astype(dtype)


def bin_image(H, W):
    """-> (H, W) int64 in fft2's layout: round(sqrt((ky L/H)^2 + (kx L/W)^2)) of the signed frequencies"""
    L = max(H, W)
    ky, kx = np.fft.fftfreq(H) * L, np.fft.fftfreq(W) * L      # cycles per L pixels: integers times L/H, L/W
    return np.rint(np.sqrt(ky[:, None] ** 2 + kx[None, :] ** 2)).astype(np.int64)


def bin_counts(H, W):
    """-> (n_r for r < R, the number of dropped corner coefficients)"""
    img, R = bin_image(H, W), max(H, W) // 2
    return np.array([(img == r).sum() for r in range(R)], dtype=np.int64), int((img >= R).sum())


def _sums(po, pf, c, H, W):
    img, R = bin_image(H, W), max(H, W) // 2
    out = np.zeros((R, 3), dtype=np.float64)
    for r in range(R):
        m = img == r
        out[r] = po[m].sum(dtype=np.float64), pf[m].sum(dtype=np.float64), c[m].sum(dtype=np.float64)
    m = img >= R
    return out, np.array([po[m].sum(dtype=np.float64), pf[m].sum(dtype=np.float64), c[m].sum(dtype=np.float64)])


def ref_sums(target, forecast, scale, corners=False):
    """float64: (frames, H, W) fields -> (frames, R, 3) sums P_o, P_f, C per radial bin; corners=True: also (frames, 3), the same three
    sums over the dropped coefficients (r >= R)"""
    o, f = clipped(target, scale), clipped(forecast, scale)
    n, H, W = o.shape
    out, rest = [], []
    for i in range(n):
        O, F = np.fft.fft2(o[i]), np.fft.fft2(f[i])
        s, c = _sums(np.abs(O) ** 2 / (H * W), np.abs(F) ** 2 / (H * W), (F * np.conj(O)).real / (H * W), H, W)
        out.append(s), rest.append(c)
    return (np.stack(out), np.stack(rest)) if corners else np.stack(out)


def ref_sums_f32(target, forecast, scale):
    """the float32 restatement: the transform in complex64 (scipy.fft), the per-coefficient products in float32, the bin sums in float64"""
    import scipy.fft
    o, f = clipped(target, scale, np.float32), clipped(forecast, scale, np.float32)
    n, H, W = o.shape
    out = []
    for i in range(n):
        O, F = scipy.fft.fft2(o[i]), scipy.fft.fft2(f[i])
        assert O.dtype == np.complex64
        inv = np.float32(1.0 / (H * W))
        po, pf = (O.real * O.real + O.imag * O.imag) * inv, (F.real * F.real + F.imag * F.imag) * inv
        c = (F.real * O.real + F.imag * O.imag) * inv
        assert po.dtype == np.float32
        out.append(_sums(po, pf, c, H, W)[0])
    return np.stack(out)


def deviation(got, ref):
    """-> (largest per-bin relative deviation, largest per-bin deviation relative to the frame's total power): the powers relative to
    themselves, the co-spectrum C relative to sqrt(P_o P_f) of its bin; the second figure relative to the frame's sum of P_o, P_f and
    sqrt(sum P_o sum P_f) respectively"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.stack([ref[..., 0], ref[..., 1], np.sqrt(ref[..., 0] * ref[..., 1])], axis=-1)
    tot = scale[..., :2].sum(axis=-2, keepdims=True)
    total = np.concatenate([tot, np.sqrt(tot[..., :1] * tot[..., 1:2])], axis=-1)
    err = np.abs(got - ref)
    return float((err / scale).max()), float((err / total).max())
