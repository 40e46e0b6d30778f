"""The flow advection without a GPU: the CPU yardstick (flow_ref) on hand-made tables and fields, its tie to the block scheme
(advect_ref), the quality conditions it is built for (asserted on the yardstick alone, so that the GPU comparison cannot be vacuous;
the figures are in profiles/flow_error.txt), the entry points at the C boundary and the Validator's arguments."""
import ctypes

import numpy as np
import pytest

import advect_ref as A
import flow_ref as F
from adnm_hip import lib

NEW = ("adnm_trec_flow_ws_bytes", "adnm_trec_flow", "adnm_flow_field", "adnm_advect_flow")


# ------------------------------------------------------------------------------------------------ 1. refinement on hand-made tables
def _valley(radius, at, cm, c0, cp, axis, high=1000):
    """a (D, D) table that is `high` everywhere but for c0 at `at` = (dy, dx) and cm, cp at its two neighbours along `axis`"""
    D = 2 * radius + 1
    t = np.full((D, D), high, dtype=np.int64)
    iy, ix = at[0] + radius, at[1] + radius
    t[iy, ix] = c0
    step = (1, 0) if axis == 0 else (0, 1)
    if 0 <= iy - step[0] and 0 <= ix - step[1]:
        t[iy - step[0], ix - step[1]] = cm
    if iy + step[0] < D and ix + step[1] < D:
        t[iy + step[0], ix + step[1]] = cp
    return t


def test_refinement_on_hand_made_tables():
    R = 3
    # a symmetric valley gives 0 on that axis; the other axis sees (high, c0, high): symmetric too
    t = _valley(R, (1, -2), 40, 10, 40, axis=0)
    assert tuple(A.pick(t, R)) == (1, -2) and F.refine(t, (1, -2), R) == (16, -32)
    # cm > cp: the minimum lies towards +1.  num = 8 * 30 = 240, den = 60 - 20 + 30 = 70: 240 / 70 = 3.43 -> 3
    t = _valley(R, (0, 0), 60, 10, 30, axis=1)
    assert F.refine(t, (0, 0), R) == (0, 3)
    assert F.refine(t.T.copy(), (0, 0), R) == (3, 0)
    # num = 8 * 10 = 80, den = 23 - 20 + 13 = 16: exactly 5
    t = _valley(R, (-1, 1), 23, 10, 13, axis=0)
    assert F.refine(t, (-1, 1), R) == (-16 + 5, 16)
    # an exact half rounds away from zero, on both sides.  den = 29 - 20 + 23 = 32 = 27 - 20 + 25 = 31 - 20 + 21
    assert F.delta(29, 10, 23, False) == 2 and F.delta(23, 10, 29, False) == -2, "48 / 32 = 1.5"
    assert F.delta(27, 10, 25, False) == 1 and F.delta(25, 10, 27, False) == -1, "16 / 32 = 0.5"
    assert F.delta(31, 10, 21, False) == 3 and F.delta(21, 10, 31, False) == -3, "80 / 32 = 2.5"
    assert F.delta(28, 10, 24, False) == 1 and F.delta(30, 10, 22, False) == 2, "32 / 32 and 64 / 32: exact"
    assert F.delta(11, 10, 13, False) == -4 and F.delta(13, 10, 11, False) == 4      # 16 / 4: exact
    assert F.delta(10, 10, 30, False) == -8 and F.delta(30, 10, 10, False) == 8, "the largest step: half a pixel"
    # den <= 0: a flat table and a ridge (cannot come from a minimal c0, but the rule is stated for every table)
    assert F.delta(10, 10, 10, False) == 0 and F.delta(5, 10, 5, False) == 0 and F.delta(5, 10, 15, False) == 0
    assert F.refine(np.zeros((2 * R + 1, 2 * R + 1), dtype=np.int64), (0, 0), R) == (0, 0)
    # a pick at the edge of the range is not refined on that axis, and is on the other
    t = _valley(R, (R, 0), 500, 10, 0, axis=0)
    t[2 * R, R - 1], t[2 * R, R + 1] = 60, 30
    assert tuple(A.pick(t, R)) == (R, 0) and F.refine(t, (R, 0), R) == (16 * R, 3)
    t = _valley(R, (0, -R), 0, 10, 500, axis=1)
    t[R - 1, 0], t[R + 1, 0] = 30, 60
    assert F.refine(t, (0, -R), R) == (-3, -16 * R)
    # |delta| <= 8 whenever c0 is the smallest of the three
    rng = np.random.default_rng(0)
    for cm, c0, cp in rng.integers(0, 1 << 33, (2000, 3)):
        lo = min(cm, c0, cp)
        assert abs(F.delta(cm, lo, cp, False)) <= 8


def test_an_invalid_block_takes_the_refined_global_vector():
    """block 0 has 32 echo pixels and moves by (0, -1); blocks 1 and 2 hold 9 brighter pixels each that move by (-1, 0) and are not
    valid (frames like those of test_advect_gpu's tie rule): they take g refined on the SUM table, not their own refinement"""
    prev, last = np.zeros((1, 16, 48), dtype=np.float32), np.zeros((1, 16, 48), dtype=np.float32)
    last[0, 4:8, 4:12], prev[0, 4:8, 5:13] = 0.5, 0.5
    last[0, 2:5, 20:23], prev[0, 3:6, 20:23] = 0.9, 0.9                   # moved by (-1, 0): inside the range of radius 2
    last[0, 2:5, 36:39], prev[0, 3:6, 36:39] = 0.9, 0.7                   # the same, dimmer before: an asymmetric valley
    u, m, c, valid, g = F.flow(prev, last, A.SCALE, 16, 2, 1, with_parts=True)
    assert valid.tolist() == [[[True, False, False]]] and tuple(g[0]) == (-1, 0)
    total = c.sum(axis=(1, 2))[0]
    ug = F.refine(total, g[0], 2)
    assert u[0, 0].tolist() == [list(F.refine(c[0, 0, 0], m[0, 0, 0], 2)), list(ug), list(ug)]
    own = [F.refine(c[0, 0, b], A.pick(c[0, 0, b], 2), 2) for b in (1, 2)]
    assert ug != (-16, 0) and ug not in own, "the refined global vector differs from the integer one and from the blocks' own refinements"
    assert (np.abs(u - 16 * m) <= 8).all()


# ------------------------------------------------------------------------------------------------ 2. the field
def test_the_dense_field():
    rng = np.random.default_rng(1)
    for block in (8, 16, 32):
        # uniform u gives uniform V = 16 u, sizes that are no multiple of the block included
        for H, W in ((40, 64), (37, 53), (5, 40)):
            nby, nbx = -(-H // block), -(-W // block)
            u = np.broadcast_to(np.array([-37, 120], dtype=np.int32), (2, nby, nbx, 2))
            assert (F.field(u, block, H, W) == np.array([-37 * 16, 120 * 16])).all()
        # a frame of one block is uniform
        u = rng.integers(-136, 137, (3, 1, 1, 2)).astype(np.int32)
        V = F.field(u, block, block - 3, block)
        assert V.shape == (3, block - 3, block, 2) and (V == 16 * u[:, :, :, None].reshape(3, 1, 1, 2)).all()
        # H and W no multiples of the block: clamped in front of the first centre, between the corners' values everywhere, and equal to a
        # plain loop in Python integers at every pixel
        H, W = 2 * block + 5, 3 * block + 1
        u = rng.integers(-136, 137, (2, 3, 4, 2)).astype(np.int32)
        V = F.field(u, block, H, W).astype(np.int64)
        assert (V[:, :block // 2, :block // 2] == 16 * u[:, :1, :1]).all(), "clamped in front of the first centre"
        assert (V >= 16 * u.min(axis=(1, 2))[:, None, None]).all() and (V <= 16 * u.max(axis=(1, 2))[:, None, None]).all()
        for y in range(H):
            for x in range(W):
                assert tuple(V[0, y, x]) == _loop_vector(u[0], block, y, x), (block, y, x)
        assert len(np.unique(V[0, :, :, 0])) > block, "nothing is interpolated"


def _axis(y, nb, block):
    p = 2 * y + 1 - block
    b0 = min(max(p // (2 * block), 0), nb - 1)
    w1 = 0 if p < 0 else min(max(p - 2 * block * b0, 0), 2 * block)
    return b0, min(b0 + 1, nb - 1), 2 * block - w1, w1


def _loop_vector(u, block, y, x):
    y0, y1, wy0, wy1 = _axis(y, u.shape[0], block)
    x0, x1, wx0, wx1 = _axis(x, u.shape[1], block)
    out = []
    for c in range(2):
        S = sum(wy * wx * 16 * int(u[by, bx, c]) for by, wy in ((y0, wy0), (y1, wy1)) for bx, wx in ((x0, wx0), (x1, wx1)))
        out.append((S + 2 * block * block) // (4 * block * block))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ 3. transport
@pytest.mark.parametrize("block,radius", A.CONFIGS)
def test_uniform_whole_pixel_flow_equals_the_block_scheme_bit_for_bit(block, radius):
    """this ties the new definition to the existing one: u = 16 v, the same v in every block, gives V = 256 v everywhere, D_t = 256 t v,
    whole-pixel sources, and a copy of the bit pattern (NaN payloads included) or +0.0 outside: advect_ref.advect"""
    case = (3, 37, 53, 4)
    _, last = A.two_motion_fields(*case)
    last = last.copy()
    last[0, 3, 5], last[1, 30, 50], last[2, 0, 0] = np.nan, np.inf, -np.inf
    last.view(np.int32)[0, 20, 20] = 0x7fc01234
    n, H, W = last.shape
    nby, nbx = -(-H // block), -(-W // block)
    for v in ((0, 0), (1, -2), (-radius, radius), (3, 0)):
        m = np.broadcast_to(np.array(v, dtype=np.int32), (n, nby, nbx, 2))
        for T in (1, 6):
            got, want = F.advect(last, 16 * m, block, T), A.advect(last, m, block, T)
            assert (got.view(np.int32) == want.view(np.int32)).all(), (v, T)


def test_a_tap_of_weight_zero_is_not_read():
    last = np.zeros((1, 8, 8), dtype=np.float32)
    last[0] = np.arange(64, dtype=np.float32).reshape(8, 8)
    last[0, 3, 4], last[0, 4, 3], last[0, 4, 4] = np.nan, np.inf, np.nan              # right of, below and diagonal to (3, 3)
    y, x = (np.broadcast_to(a[None], (1, 8, 8)) for a in np.mgrid[0:8, 0:8].astype(np.int64))
    whole = F.interpolate(last, 256 * y, 256 * x)
    assert (whole.view(np.int32) == last.view(np.int32)).all(), "zero motion is a copy"
    half_x = F.interpolate(last, 256 * y, 256 * x + 128)                               # fy == 0: rows 4 of the taps are never read
    assert half_x[0, 3, 2] == np.float32(0.5) * 26 + np.float32(0.5) * 27 and np.isnan(half_x[0, 3, 3]) and not np.isnan(half_x[0, 2, 3])
    assert not np.isinf(half_x[0, 3, 2]) and np.isfinite(half_x[0, 2]).all(), "the row below does not leak through fy == 0"
    half_y = F.interpolate(last, 256 * y + 64, 256 * x)                                # fx == 0: column x + 1 is never read
    assert np.isfinite(half_y[0, :, 2]).all() and half_y[0, 2, 2] == np.float32(0.75) * 18 + np.float32(0.25) * 26
    assert np.isinf(half_y[0, 3, 3]) and np.isnan(half_y[0, 2, 4]), "a tap with a weight does count"
    # outside the frame is +0.0: the last column read half a pixel to the right is half its value
    assert (half_x[0, :3, 7] == np.float32(0.5) * last[0, :3, 7]).all()
    # the order of the roundings: products first, each rounded, then the sum
    a, b, fx = np.float32(0.1), np.float32(0.7), np.float32(3 / 256)
    last2 = np.array([[[a, b]]], dtype=np.float32)
    got = F.interpolate(last2, np.zeros((1, 1, 2), dtype=np.int64), np.array([[[3, 256]]], dtype=np.int64))
    assert got[0, 0, 0] == np.float32(np.float32((np.float32(1) - fx) * a) + np.float32(fx * b)) and got[0, 0, 1] == b


def test_transport_follows_the_field_step_by_step():
    """two halves with different whole-pixel vectors: a pixel that crosses the seam changes its step there (the block scheme keeps its
    block's vector however far it has travelled)"""
    block, H, W = 8, 8, 32
    u = np.zeros((1, 1, 4, 2), dtype=np.int32)
    u[0, 0, :2, 1], u[0, 0, 2:, 1] = 16 * 2, 16 * 4                                     # ux = 2 px on the left, 4 px on the right
    last = np.arange(H * W, dtype=np.float32).reshape(1, H, W)
    out, D = F.advect(last, u, block, 3, with_displacement=True)
    V = F.field(u, block, H, W)
    assert (V[0, :, :12, 1] == 512).all() and (V[0, :, 20:, 1] == 1024).all() and (np.diff(V[0, 0, :, 1]) >= 0).all()
    assert D[0, 0, 5, 1] == 3 * 512 and D[0, 0, 31, 1] == 1024 + 1024 + 1024 and D[0, 0, 22, 1] == 1024 + V[0, 0, 18, 1] + V[0, 0, 22 - 4 - (V[0, 0, 18, 1] + 128) // 256, 1]
    assert out[0, 2, 0, 5] == 0.0 and out[0, 0, 0, 5] == last[0, 0, 3] and out[0, 2, 0, 31] == last[0, 0, 19]


# ------------------------------------------------------------------------------------------------ 4. the quality conditions
def test_the_flow_is_closer_to_the_truth_than_the_block_scheme_on_the_yardstick():
    """no numeric bar: the comparison is against the block scheme on the same inputs, strictly, at every (block, radius) used.  The
    figures are flow_ref.quality_report's; `python tests/flow_ref.py` writes them to profiles/flow_error.txt"""
    text, shifts, rotations = F.quality_report()
    print(text)
    assert len(shifts) == len(F.SHIFT_CASES) * len(A.CONFIGS) and len(rotations) == len(F.ROTATION_SEEDS) * len(A.CONFIGS)
    for what, fine, coarse, nvalid in shifts:
        assert nvalid >= 8 and fine < coarse, f"{what}: refined {fine} integer {coarse} ({nvalid} valid blocks): pick another seed, do not weaken this"
    for what, e_flow, e_block, e_hold in rotations:
        assert e_flow < e_block < e_hold, f"{what}: flow {e_flow} block scheme {e_block} persistence {e_hold}: pick another seed, do not weaken this"


@pytest.mark.parametrize("block,radius", A.CONFIGS)
def test_the_listed_cases_exercise_the_refinement(block, radius):
    """what test_flow_gpu compares is not vacuous: every case has a block with a non-zero delta on each axis; the cases together have a
    refinement refused at the edge of the range and an invalid block"""
    print(F.assert_refined(A.CASES, block, radius))
    still = np.zeros((1, 16, 16), dtype=np.float32)
    with pytest.raises(AssertionError, match="do not weaken this$"):
        F.assert_refined(["two empty frames"], block, radius, fields=lambda case: (still, still))


# ------------------------------------------------------------------------------------------------ 5. the C boundary
def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_trec_flow_ws_bytes"] == ("int64_t", ["int64_t"] * 5)
    assert protos["adnm_trec_flow"] == protos["adnm_trec_motion"], "one call shape for both schemes' estimates"
    assert protos["adnm_advect_flow"] == protos["adnm_advect"], "and for both transports"
    assert protos["adnm_flow_field"] == ("int", ["const void*", "void*"] + ["int64_t"] * 4 + ["adnm_stream_t"])
    assert lib.load().adnm_abi_version() == 11
    for shape in ((4, 128, 128, 32, 4), (3, 37, 53, 8, 2), (1, 1, 1, 16, 1)):
        assert lib.query("adnm_trec_flow_ws_bytes", *shape) == lib.query("adnm_trec_ws_bytes", *shape) > 0
    for bad in ((0, 64, 64, 16, 4), (2, 64, 64, 12, 4), (2, 64, 64, 16, 9), (2, 4096, 4096, 16, 4), (65536, 64, 64, 16, 4)):
        assert lib.query("adnm_trec_flow_ws_bytes", *bad) == -1, bad


def test_every_limit_is_refused_on_the_host_with_its_own_message():
    """fake addresses: anything that reached a launch would fault, and the stream is never touched"""
    so = lib.load()

    def flow(prev=16, last=32, ss=64 * 64, u=64, mot=None, scale=90.0, block=16, radius=4, echo=20, ws=128, ws_bytes=1 << 30, samples=2, H=64, W=64):
        return so.adnm_trec_flow(prev, last, ss, u, mot, scale, block, radius, echo, ws, ws_bytes, samples, H, W, None), lib.last_error()

    def field(u=64, out=96, block=16, samples=2, H=64, W=64):
        return so.adnm_flow_field(u, out, block, samples, H, W, None), lib.last_error()

    def advect(last=32, ss=64 * 64, u=64, out=96, block=16, samples=2, T=5, H=64, W=64):
        return so.adnm_advect_flow(last, ss, u, out, block, samples, T, H, W, None), lib.last_error()

    shape = [(dict(block=4), "8, 16 or 32"), (dict(block=24), "8, 16 or 32"), (dict(samples=0), "1..65535"), (dict(samples=65536), "1..65535"),
             (dict(H=0), "[1, 32768)"), (dict(W=32768, H=16), "[1, 32768)"), (dict(H=4096, W=4096), "2^24")]
    cases = [(dict(prev=None), "null pointer"), (dict(last=None), "null pointer"), (dict(u=None), "null pointer"),
             (dict(prev=18), "prev and last must be 4-byte aligned"), (dict(u=66), "flow and motion must be 4-byte aligned"),
             (dict(mot=130), "flow and motion must be 4-byte aligned"), (dict(radius=0), "radius"), (dict(radius=9), "radius"),
             (dict(echo=0), "echo"), (dict(echo=256), "echo"), (dict(scale=0.0), "value_scale"), (dict(scale=255.5), "value_scale"),
             (dict(scale=float("nan")), "value_scale"), (dict(ss=64 * 64 - 1), "sample_stride")] + [(dict(kw, ss=1 << 24), text) for kw, text in shape]
    for kw, text in cases:
        rc, err = flow(**kw)
        assert rc == -1 and text in err and "trec_flow" in err, (kw, rc, err)
    assert flow(ws_bytes=8)[0] == -3 and "workspace" in lib.last_error() and flow(ws=None)[0] == -3
    assert flow(ws_bytes=lib.query("adnm_trec_flow_ws_bytes", 2, 64, 64, 16, 4) - 1)[0] == -3
    for kw, text in [(dict(u=None), "null pointer"), (dict(out=None), "null pointer"), (dict(u=66), "4-byte aligned"), (dict(out=98), "4-byte aligned")] + shape:
        rc, err = field(**kw)
        assert rc == -1 and text in err and "flow_field" in err, (kw, rc, err)
    cases = [(dict(last=None), "null pointer"), (dict(u=None), "null pointer"), (dict(out=None), "null pointer"),
             (dict(last=34), "last and out must be 4-byte aligned"), (dict(out=98), "last and out must be 4-byte aligned"), (dict(u=66), "flow must be 4-byte aligned"),
             (dict(T=0), "T must be in 1..4096"), (dict(T=-3), "T must be in 1..4096"), (dict(T=4097), "T must be in 1..4096"),
             (dict(ss=64 * 64 - 1), "sample_stride")] + [(dict(kw, ss=1 << 24), text) for kw, text in shape]
    for kw, text in cases:
        rc, err = advect(**kw)
        assert rc == -1 and text in err and "advect_flow" in err, (kw, rc, err)


# ------------------------------------------------------------------------------------------------ 6. the arguments
def test_validator_arguments():
    import inspect

    import torch
    from adnm_hip import ops
    from adnm_hip.validate import Validator, block_parts
    from models.loss import enRainfallLoss
    assert inspect.signature(Validator.__init__).parameters["advection_flow"].default is False
    model, crit = torch.nn.Identity(), enRainfallLoss()
    plain = Validator(model, crit, 20, 255.0, advection=(16, 4), persistence=True, pools=(4,), fss=9)
    val = Validator(model, crit, 20, 255.0, advection=(16, 4), persistence=True, pools=(4,), fss=9, advection_flow=True)
    assert plain.advection_flow is False and val.advection_flow is True and val.advection == plain.advection == (16, 4, 10)
    assert val._parts == plain._parts == block_parts(20, 4, ((4, 4),), True, (9,), True)[0], "the flag moves no table"
    for none in (None, False):
        with pytest.raises(ValueError, match="advection_flow"):
            Validator(model, crit, 20, 255.0, advection=none, advection_flow=True)
    with pytest.raises(ValueError, match="advection_flow"):
        Validator(model, crit, 20, 255.0, advection_flow=True)
    with pytest.raises(ValueError, match=str(ops.MAX_FLOW_T)):
        Validator(model, crit, ops.MAX_FLOW_T + 1, 255.0, advection=True, advection_flow=True)
    Validator(model, crit, ops.MAX_FLOW_T + 1, 255.0, advection=True)
    with pytest.raises(ValueError, match="value_scale <= 255"):
        Validator(model, crit, 20, 256.0, advection=True, advection_flow=True)
    for v in (val, plain):
        with pytest.raises(RuntimeError, match="flow"):
            v.flow(torch.zeros(1, 5, 1, 8, 8))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.extrapolate(torch.zeros(1, 5, 8, 8), 3, 255.0)
