"""The CPU yardstick of the flow advection (csrc/flow.hip: adnm_trec_flow, adnm_flow_field, adnm_advect_flow), written
differently from the kernels: the sub-pixel refinement by plain Python loops over the blocks on Python integers, the dense field by
gathered corner arrays, the transport by whole-array index arithmetic in int64 with the interpolation in np.float32, every product and
every sum rounded on its own, in the stated order.  It builds on advect_ref.costs / pick / motion: the integer pick, the global pick and
the validity are the block scheme's.  Everything up to the four taps is integer arithmetic: u and V compare integer for integer, the
advected field bit for bit.  The reference project has no motion estimate, so nothing here is recorded from it.

Also the two synthetic fields the quality conditions are stated on (fractional shifts, solid-body rotation) with their analytic truth."""
import numpy as np

import advect_ref as A
import verify_ref as R

MAX_T = 4096
# (n, H, W, seed) of shifted_blobs and the fractional shifts (dy, dx) in px per frame; seeds of rotating_blobs (128 x 128, 0.03 rad per
# frame, 10 leads).  The seeds are the first, counting up from 0, at which the quality condition (the refined vectors are closer to the
# truth than the integer pick; the flow advection is closer to the truth than the block advection) holds at all three advect_ref.CONFIGS.
SHIFT_CASES = [(2, 96, 96, 0), (2, 96, 96, 1), (2, 96, 96, 2)]
SHIFTS = [(1.5, -0.5), (0.25, 1.75), (-1.3, 0.6)]
ROTATION_SEEDS = [0, 1, 2]
ROTATION = dict(size=128, omega=0.03, leads=10)


# ------------------------------------------------------------------------------------------------ 1. refinement
def delta(cm, c0, cp, at_edge):
    """one axis: the parabola through (-1, cm), (0, c0), (1, cp) has its vertex at (cm - cp) / (2 den), den = cm - 2 c0 + cp; in 1/16 px
    that is 8 (cm - cp) / den, rounded half away from zero.  0 at the edge of the range and where the parabola does not open upwards."""
    cm, c0, cp = int(cm), int(c0), int(cp)
    den = cm - 2 * c0 + cp
    if at_edge or den <= 0:
        return 0
    num = 8 * (cm - cp)
    mag = (2 * abs(num) + den) // (2 * den)
    return mag if num > 0 else -mag


def refine(table, d, radius):
    """table: (D, D) costs, d: its pick (dy, dx) -> (uy, ux) in 1/16 px"""
    dy, dx = int(d[0]), int(d[1])
    iy, ix = dy + radius, dx + radius
    ey, ex = abs(dy) == radius, abs(dx) == radius
    ty = delta(0 if ey else table[iy - 1, ix], table[iy, ix], 0 if ey else table[iy + 1, ix], ey)
    tx = delta(0 if ex else table[iy, ix - 1], table[iy, ix], 0 if ex else table[iy, ix + 1], ex)
    return 16 * dy + ty, 16 * dx + tx


def flow(prev, last, scale, block, radius, echo, with_parts=False):
    """-> int32 (n, nby, nbx, 2), the block flow u in 1/16 px: a valid block refines its own pick on its own table, an invalid block takes
    the global pick refined on the sum table.  with_parts: -> (u, motion, costs, valid, g)"""
    m, c, valid, g = A.motion(prev, last, scale, block, radius, echo, with_parts=True)
    n, nby, nbx = valid.shape
    total = c.sum(axis=(1, 2))
    u = np.zeros((n, nby, nbx, 2), dtype=np.int32)
    for s in range(n):
        ug = refine(total[s], g[s], radius)
        for by in range(nby):
            for bx in range(nbx):
                u[s, by, bx] = refine(c[s, by, bx], m[s, by, bx], radius) if valid[s, by, bx] else ug
    return (u, m, c, valid, g) if with_parts else u


def refused_at_the_edge(m, valid, g, radius):
    """the number of (block, axis) pairs whose refinement is refused because the pick lies at the edge of the range"""
    v = np.where(valid[..., None], m, g[:, None, None, :])
    return int((np.abs(v) == radius).sum())


def assert_refined(cases, block, radius, scale=A.SCALE, fields=None):
    """a test may not hide a failure by comparing nothing.  On every listed case the CPU reference alone shows, at echo = 1 and at
    echo = advect_ref.ECHO, a block with delta != 0 on each axis; over the cases of one (block, radius) together at least one refinement
    refused at the edge of the range and at least one invalid block.  fields: case -> (prev, last), advect_ref.two_motion_fields by default.
    -> (refused, invalid) over the cases"""
    refused = invalid = 0
    for case in cases:
        prev, last = A.two_motion_fields(*case) if fields is None else fields(case)
        for echo in (1, A.ECHO):
            u, m, _, valid, g = flow(prev, last, scale, block, radius, echo, with_parts=True)
            moved = u != 16 * np.where(valid[..., None], m, g[:, None, None, :])
            assert moved[..., 0].any() and moved[..., 1].any(), (f"{case} block {block} radius {radius} echo {echo}: no block of the CPU reference is refined "
                                                                 "on one of the axes: pick another seed, do not weaken this")
            refused += refused_at_the_edge(m, valid, g, radius)
            invalid += int((~valid).sum())
    assert refused >= 1, f"block {block} radius {radius}: no pick at the edge of the range in the CPU reference of {cases}: pick another seed, do not weaken this"
    assert invalid >= 1, f"block {block} radius {radius}: no invalid block in the CPU reference of {cases}: pick another seed, do not weaken this"
    return refused, invalid


# ------------------------------------------------------------------------------------------------ 2. the dense field
def axis_weights(N, nb, block):
    """-> (b0, b1, w0, w1), int64 arrays of length N: the two block centres around pixel y and their integer weights (sum 2 block)"""
    p = 2 * np.arange(N, dtype=np.int64) + 1 - block
    b0 = np.clip(np.floor_divide(p, 2 * block), 0, nb - 1)
    b1 = np.minimum(b0 + 1, nb - 1)
    w1 = np.where(p < 0, 0, np.clip(p - 2 * block * b0, 0, 2 * block))
    return b0, b1, 2 * block - w1, w1


def field(u, block, H, W):
    """u: (n, nby, nbx, 2) in 1/16 px -> V int32 (n, H, W, 2) in 1/256 px, bilinear between the block centres, clamped at the outermost"""
    u = np.asarray(u, dtype=np.int64)
    n, nby, nbx, _ = u.shape
    assert (nby, nbx) == (-(-H // block), -(-W // block))
    y0, y1, wy0, wy1 = (a[:, None] for a in axis_weights(H, nby, block))
    x0, x1, wx0, wx1 = (a[None, :] for a in axis_weights(W, nbx, block))
    S = np.zeros((n, H, W, 2), dtype=np.int64)
    for by, wy in ((y0, wy0), (y1, wy1)):
        for bx, wx in ((x0, wx0), (x1, wx1)):
            S += (wy * wx)[None, :, :, None] * 16 * u[:, by, bx]            # the gathered corner, (n, H, W, 2)
    V = np.floor_divide(S + 2 * block * block, 4 * block * block)
    return V.astype(np.int32)


# ------------------------------------------------------------------------------------------------ 3. transport
def _taps(last, iy, ix, need):
    """last: (n, H, W) fp32; iy, ix: (n, H, W) int64 -> last[s, iy, ix], +0.0 outside the frame and where `need` is False (not read)"""
    n, H, W = last.shape
    ok = need & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    flat = np.where(ok, iy * W + ix, 0).reshape(n, -1)
    got = np.take_along_axis(last.reshape(n, -1).view(np.int32), flat, axis=1).reshape(n, H, W)
    return np.where(ok, got, np.int32(0)).astype(np.int32).view(np.float32)


def interpolate(last, sy, sx):
    """sy, sx: (n, H, W) int64 source positions in 1/256 px -> fp32 (n, H, W), the four taps combined in np.float32 in the stated order.
    A tap of weight 0 is not read: fx == 0 gives top = a, fy == 0 gives out = top."""
    iy, ix = sy >> 8, sx >> 8
    ky, kx = sy - 256 * iy, sx - 256 * ix
    fy, fx = (ky.astype(np.float32) / np.float32(256)), (kx.astype(np.float32) / np.float32(256))
    gy, gx = np.float32(1) - fy, np.float32(1) - fx
    yes, right, below = np.ones(iy.shape, dtype=bool), kx != 0, ky != 0
    a, b = _taps(last, iy, ix, yes), _taps(last, iy, ix + 1, right)
    c, d = _taps(last, iy + 1, ix, below), _taps(last, iy + 1, ix + 1, below & right)
    with np.errstate(invalid="ignore", over="ignore"):
        top = np.where(right, (gx * a).astype(np.float32) + (fx * b).astype(np.float32), a).astype(np.float32)
        bot = np.where(right, (gx * c).astype(np.float32) + (fx * d).astype(np.float32), c).astype(np.float32)
        mix = ((gy * top).astype(np.float32) + (fy * bot).astype(np.float32)).astype(np.float32)
    return np.where(below, mix.view(np.int32), top.view(np.int32)).astype(np.int32).view(np.float32)     # (selected as bits: a copy stays a copy)


def advect(last, u, block, T, with_displacement=False):
    """last: (n, H, W) fp32; u: (n, nby, nbx, 2) in 1/16 px -> fp32 (n, T, H, W): backward semi-Lagrangian transport along the dense field,
    one step per frame, the departure point followed in 1/256 px"""
    assert 1 <= T <= MAX_T
    last = np.ascontiguousarray(last, dtype=np.float32)
    n, H, W = last.shape
    V = field(u, block, H, W).astype(np.int64)
    y, x = (np.broadcast_to(a[None], (n, H, W)) for a in np.mgrid[0:H, 0:W].astype(np.int64))
    s_ix = np.arange(n)[:, None, None]
    Dy, Dx = np.zeros((n, H, W), dtype=np.int64), np.zeros((n, H, W), dtype=np.int64)
    out = np.zeros((n, T, H, W), dtype=np.float32)
    for t in range(T):
        ry = np.clip((256 * y - Dy + 128) >> 8, 0, H - 1)
        rx = np.clip((256 * x - Dx + 128) >> 8, 0, W - 1)
        step = V[s_ix, ry, rx]
        Dy, Dx = Dy + step[..., 0], Dx + step[..., 1]
        out[:, t] = interpolate(last, 256 * y - Dy, 256 * x - Dx)
    return (out, np.stack([Dy, Dx], axis=-1)) if with_displacement else out


def same_bits_or_both_nan(got, want):
    """-> the number of cells where `got` is neither bit-equal to `want` nor a NaN where `want` is one"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return int((np.where(nan, ~np.isnan(got), got.view(np.int32) != want.view(np.int32))).sum())


# ------------------------------------------------------------------------------------------------ 4. the fields of the quality conditions
def _gauss(H, W, cy, cx, amp, sig):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return (amp[:, None, None] * np.exp(-((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2) / (2 * sig[:, None, None] ** 2))).sum(axis=0)


def _blob_set(rng, H, W, count, margin):
    return (rng.uniform(margin, H - margin, count), rng.uniform(margin, W - margin, count), rng.uniform(0.25, 0.62, count), rng.uniform(3.0, 7.0, count))


def shifted_blobs(n, H, W, seed, shift, count=8):
    """-> (prev, last), (n, H, W) fp32: smooth blob fields (analytic Gaussians, no noise) whose every blob moves by the fractional `shift`
    = (dy, dx) px per frame: the truth of every block is `shift`"""
    rng = np.random.default_rng(seed)
    prev, last = np.zeros((n, H, W)), np.zeros((n, H, W))
    for s in range(n):
        cy, cx, amp, sig = _blob_set(rng, H, W, count, 0.0)
        prev[s], last[s] = _gauss(H, W, cy, cx, amp, sig), _gauss(H, W, cy + shift[0], cx + shift[1], amp, sig)
    return prev.astype(np.float32), last.astype(np.float32)


def rotating_blobs(seed, size=128, omega=0.03, leads=10, count=10):
    """-> (prev, last, truth): (1, size, size) fp32 frames at steps -1 and 0 and (1, leads, size, size) at steps 1 .. leads of a blob field
    in solid-body rotation by `omega` rad per frame about the frame's centre (isotropic Gaussians: rotating the centres rotates the field)"""
    rng = np.random.default_rng(seed)
    cy, cx, amp, sig = _blob_set(rng, size, size, count, 0.15 * size)
    c = (size - 1) / 2.0

    def frame(step):
        co, si = np.cos(omega * step), np.sin(omega * step)
        return _gauss(size, size, c + co * (cy - c) - si * (cx - c), c + si * (cy - c) + co * (cx - c), amp, sig)
    truth = np.stack([frame(k) for k in range(1, leads + 1)])[None]
    return frame(-1)[None].astype(np.float32), frame(0)[None].astype(np.float32), truth.astype(np.float32)


def vector_errors(prev, last, shift, scale, block, radius, echo):
    """-> (mean |u / 16 - shift|, mean |d - shift|) in px over the valid blocks, and their number"""
    u, m, _, valid, _ = flow(prev, last, scale, block, radius, echo, with_parts=True)
    truth = np.asarray(shift, dtype=np.float64)
    fine = np.linalg.norm(u[valid] / 16.0 - truth, axis=-1)
    coarse = np.linalg.norm(m[valid].astype(np.float64) - truth, axis=-1)
    return float(fine.mean()), float(coarse.mean()), int(valid.sum())


def rotation_errors(seed, scale, block, radius, echo):
    """-> (flow, block, persistence): the absolute error against the truth summed over the leads and the pixels"""
    prev, last, truth = rotating_blobs(seed, **ROTATION)
    T = truth.shape[1]
    u, m, _, _, _ = flow(prev, last, scale, block, radius, echo, with_parts=True)
    err = lambda f: float(np.abs(f.astype(np.float64) - truth).sum())      # noqa: E731
    return err(advect(last, u, block, T)), err(A.advect(last, m, block, T)), err(np.broadcast_to(last[:, None], truth.shape))


def quality_report():
    """-> (text, [(what, refined, integer, valid blocks)], [(what, flow, block scheme, persistence)]): the figures of the quality conditions
    at every advect_ref.CONFIGS, at echo = advect_ref.ECHO of advect_ref.SCALE"""
    lines = [f"flow advection against the block scheme on the CPU yardstick (tests/flow_ref.py; value_scale {A.SCALE:g}, echo {A.ECHO})", "",
             "fractional shifts: mean vector error of the valid blocks in px, refined (u / 16) and integer pick"]
    shifts, rotations = [], []
    for case, shift in zip(SHIFT_CASES, SHIFTS):
        prev, last = shifted_blobs(*case, shift)
        for block, radius in A.CONFIGS:
            fine, coarse, nvalid = vector_errors(prev, last, shift, A.SCALE, block, radius, A.ECHO)
            shifts.append((f"case {case} shift {shift} block {block:2d} radius {radius}", fine, coarse, nvalid))
            lines.append(f"  {shifts[-1][0]}: refined {fine:.3f}  integer {coarse:.3f}  ({nvalid} valid blocks)")
    lines += ["", f"solid-body rotation, {ROTATION['size']} x {ROTATION['size']}, {ROTATION['omega']} rad per frame, {ROTATION['leads']} leads: "
              "summed absolute error against the truth"]
    for seed in ROTATION_SEEDS:
        for block, radius in A.CONFIGS:
            e = rotation_errors(seed, A.SCALE, block, radius, A.ECHO)
            rotations.append((f"seed {seed} block {block:2d} radius {radius}",) + e)
            lines.append(f"  {rotations[-1][0]}: flow {e[0]:7.0f}  block scheme {e[1]:7.0f}  persistence {e[2]:7.0f}")
    return "\n".join(lines) + "\n", shifts, rotations


if __name__ == "__main__":          # python tests/flow_ref.py: the figures for the record
    import os
    report = quality_report()[0]
    print(report)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flow_error.txt"), "w") as out:
        out.write(report)
