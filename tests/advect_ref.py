"""The CPU yardstick of the advection baseline (csrc/advect.hip: adnm_trec_motion, adnm_advect): block-matching costs by slicing the
zero-padded quantised previous frame once per displacement and summing |differences| per block, the pick by argmin of one packed integer
key, the advected field by index arithmetic and a gather of bit patterns.  Everything is integer arithmetic or a bit copy: every
comparison against this reference is exact.  The reference project has no motion estimate, so nothing here is recorded from it."""
import numpy as np

import verify_ref as R

SCALE = R.SCALE
ECHO = 20                      # of SCALE = 90: the echo count the density conditions are stated at
CONFIGS = [(8, 2), (16, 4), (32, 8)]          # (block, radius)
# (samples, H, W, seed) of two_motion_fields: whole tiles with 16-byte loads, odd sizes with clipped edge blocks on both axes, a frame
# thinner than one block, a frame that is a single block.  The seeds are the first, counting up from 0, 1, 2, 3, 4, 5, at which the case
# meets assert_dense's per-case conditions at all three CONFIGS.
CASES = [(4, 64, 64, 0), (3, 37, 53, 4), (2, 128, 128, 2), (3, 33, 33, 4), (2, 5, 40, 42), (2, 16, 16, 9)]


def qint(v, scale):
    """verify_ref.quant as int64"""
    return R.quant(v, scale).astype(np.int64)


def _block_sums(a, block):
    """(n, H, W) int64 -> (n, nby, nbx): padded to whole blocks with zeros, reshaped, summed"""
    n, H, W = a.shape
    nby, nbx = -(-H // block), -(-W // block)
    p = np.zeros((n, nby * block, nbx * block), dtype=np.int64)
    p[:, :H, :W] = a
    return p.reshape(n, nby, block, nbx, block).sum(axis=(2, 4))


def costs(prev, last, scale, block, radius):
    """prev, last: (n, H, W) float arrays -> (n, nby, nbx, D, D) int64, D = 2 radius + 1:
    [.., dy + radius, dx + radius] = sum over the block's in-frame pixels of |q(last)(y, x) - q(prev)(y - dy, x - dx)|, q(prev) = 0 outside"""
    qp, ql = qint(prev, scale), qint(last, scale)
    n, H, W = ql.shape
    Rr, D = radius, 2 * radius + 1
    pad = np.pad(qp, ((0, 0), (Rr, Rr), (Rr, Rr)))
    out = np.zeros((n, -(-H // block), -(-W // block), D, D), dtype=np.int64)
    for dy in range(-Rr, Rr + 1):
        for dx in range(-Rr, Rr + 1):
            shifted = pad[:, Rr - dy:Rr - dy + H, Rr - dx:Rr - dx + W]          # prev(y - dy, x - dx)
            out[:, :, :, dy + Rr, dx + Rr] = _block_sums(np.abs(ql - shifted), block)
    return out


def loop_costs(prev, last, scale, block, radius):
    """the same by a plain quadruple loop (the helper's self-check: small cases only)"""
    qp, ql = qint(prev, scale), qint(last, scale)
    n, H, W = ql.shape
    D = 2 * radius + 1
    out = np.zeros((n, -(-H // block), -(-W // block), D, D), dtype=np.int64)
    for s in range(n):
        for y in range(H):
            for x in range(W):
                for dy in range(-radius, radius + 1):
                    for dx in range(-radius, radius + 1):
                        py, px = y - dy, x - dx
                        p = qp[s, py, px] if 0 <= py < H and 0 <= px < W else 0
                        out[s, y // block, x // block, dy + radius, dx + radius] += abs(int(ql[s, y, x]) - int(p))
    return out


def pick(table, radius):
    """(..., D, D) int64 costs -> (..., 2) int64 (dy, dx): argmin of ((cost (2 R^2 + 1) + dy^2 + dx^2) D + dy + R) D + dx + R"""
    D = 2 * radius + 1
    dy, dx = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
    key = ((table * (2 * radius * radius + 1) + dy * dy + dx * dx) * D + dy + radius) * D + dx + radius
    at = key.reshape(key.shape[:-2] + (D * D,)).argmin(axis=-1)
    return np.stack([at // D - radius, at % D - radius], axis=-1)


def echo_counts(last, scale, block, echo):
    """-> (n, nby, nbx): the block's in-frame pixels with q(last) >= echo"""
    return _block_sums((qint(last, scale) >= echo).astype(np.int64), block)


def motion(prev, last, scale, block, radius, echo, with_parts=False):
    """-> int32 (n, nby, nbx, 2) of (vy, vx): a valid block's own pick, the sample's global vector elsewhere.
    with_parts: -> (motion, costs, valid (n, nby, nbx) bool, g (n, 2))"""
    c = costs(prev, last, scale, block, radius)
    g = pick(c.sum(axis=(1, 2)), radius)
    valid = echo_counts(last, scale, block, echo) >= block
    m = np.where(valid[..., None], pick(c, radius), g[:, None, None, :]).astype(np.int32)
    return (m, c, valid, g) if with_parts else m


def advect(last, mot, block, T):
    """last: (n, H, W) fp32, mot: (n, nby, nbx, 2) -> (n, T, H, W) fp32 whose BITS are last[s, y - (t+1) vy, x - (t+1) vx], +0.0 outside"""
    bits = np.ascontiguousarray(last, dtype=np.float32).view(np.int32)
    n, H, W = bits.shape
    y, x = np.mgrid[0:H, 0:W]
    v = np.asarray(mot, dtype=np.int64)[:, y // block, x // block]            # (n, H, W, 2)
    lead = np.arange(1, T + 1, dtype=np.int64)[None, :, None, None]
    sy, sx = y[None, None] - lead * v[:, None, :, :, 0], x[None, None] - lead * v[:, None, :, :, 1]
    inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    flat = np.where(inside, sy * W + sx, 0).reshape(n, -1)
    got = np.take_along_axis(bits.reshape(n, -1), flat, axis=1).reshape(n, T, H, W)
    return np.where(inside, got, np.int32(0)).astype(np.int32).view(np.float32)


def two_motion_fields(n, H, W, seed):
    """-> (prev, last), (n, H, W) fp32: two independent blob fields (5 blobs each) on a canvas 12 px larger on every side; the left half
    of the canvas moves by (1, 2) per frame, the right half by (-2, 0); N(0, 0.01) noise on each frame; cropped to the frame.  One vector
    for the whole frame cannot explain both halves, so the per-block pick is exercised."""
    rng = np.random.default_rng(seed)
    m = 12
    Hc, Wc = H + 2 * m, W + 2 * m
    a, b = R.blobs(rng, n, Hc, Wc, 5), R.blobs(rng, n, Hc, Wc, 5)
    half = Wc // 2

    def frame(step):
        f = np.roll(b, (-2 * step, 0), axis=(1, 2))
        f[:, :, :half] = np.roll(a, (step, 2 * step), axis=(1, 2))[:, :, :half]
        return (f + rng.normal(0.0, 0.01, size=f.shape))[:, m:m + H, m:m + W].astype(np.float32)
    return frame(0), frame(1)


def tied_blocks(c):
    """(n, nby, nbx, D, D) -> the number of blocks whose smallest cost is reached by more than one displacement"""
    flat = c.reshape(c.shape[:3] + (-1,))
    return int(((flat == flat.min(axis=-1, keepdims=True)).sum(axis=-1) > 1).sum())


def assert_dense(cases, block, radius, scale=SCALE, fields=None):
    """a test may not hide a failure by comparing nothing.  On every listed case the CPU reference alone shows, at echo = 1 and at
    echo = ECHO, at least 2 distinct vectors and a non-zero vector in every sample, and at echo = ECHO a valid block in every sample; over the cases of one
    (block, radius) together at least one tied block and at least one invalid block.  fields: case -> (prev, last), two_motion_fields by
    default.  -> (tied, invalid) over the cases"""
    tied = invalid = 0
    for case in cases:
        prev, last = two_motion_fields(*case) if fields is None else fields(case)
        what = f"{case} block {block} radius {radius}"
        m, c, valid, _ = motion(prev, last, scale, block, radius, 1, with_parts=True)
        m_echo, _, valid_echo, _ = motion(prev, last, scale, block, radius, ECHO, with_parts=True)
        tied += tied_blocks(c)
        invalid += int((~valid).sum()) + int((~valid_echo).sum())
        for echo, v in ((1, m), (ECHO, m_echo)):
            distinct = len({tuple(d) for d in v.reshape(-1, 2)})
            assert distinct >= 2, f"{what} echo {echo}: the CPU reference has {distinct} distinct vector(s): pick another seed, do not weaken this"
            assert (v != 0).any(axis=(1, 2, 3)).all(), f"{what} echo {echo}: a sample of the CPU reference has only zero vectors: pick another seed, do not weaken this"
        assert valid_echo.any(axis=(1, 2)).all(), f"{what}: a sample has no valid block at echo {ECHO}: pick another seed, do not weaken this"
    assert tied >= 1, f"block {block} radius {radius}: no tied block in the CPU reference of {cases}: pick another seed, do not weaken this"
    assert invalid >= 1, f"block {block} radius {radius}: no invalid block in the CPU reference of {cases}: pick another seed, do not weaken this"
    return tied, invalid
