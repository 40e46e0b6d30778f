"""Sub-pixel flow and transport along it on the GPU (csrc/flow.hip: adnm_trec_flow, adnm_flow_field, adnm_advect_flow; ops.trec_flow,
ops.flow_field, ops.advect_flow, ops.extrapolate; Validator(advection_flow=True)): exact against the CPU yardstick (flow_ref), the
block flow and the dense field integer for integer, the advected field bit for bit where the yardstick is not NaN and NaN where it is,
at every addressing the Validator uses, and end to end through the captured graph."""
import numpy as np
import pytest
import torch

import advect_ref as A
import flow_ref as F
import fss_ref as FS
import verify_ref as R
from adnm_hip import lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR, SCALE = R.THR, A.SCALE

_fields, _refs = {}, {}


def _pair(case):
    """the CPU frames of a case, made once and never written to"""
    if case not in _fields:
        _fields[case] = A.two_motion_fields(*case)
        for a in _fields[case]:
            a.setflags(write=False)
    return _fields[case]


def _reference(prev, last, block, radius, echo, T, scale=SCALE):
    """-> (u, motion, V, advected (n, T, H, W)) of the yardstick"""
    u, m = F.flow(prev, last, scale, block, radius, echo, with_parts=True)[:2]
    return u, m, F.field(u, block, *last.shape[-2:]), F.advect(last, u, block, T)


def _ref(case, block, radius, echo):
    """the yardstick's (u, motion, V, advected at T = 6) of a case, made once and never written to"""
    key = (case, block, radius, echo)
    if key not in _refs:
        _refs[key] = _reference(*_pair(case), block, radius, echo, 6)
        for a in _refs[key]:
            a.setflags(write=False)
    return _refs[key]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the cached fields are read-only)


def _same_field(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, what
    bad = F.same_bits_or_both_nan(got, want)
    assert bad == 0, f"{what}: {bad} of {want.size} cells are neither the yardstick's bits nor a NaN where it has one"


def _check(prev, last, block, radius, echo, Ts, ref=None, scale=SCALE):
    """ops against the yardstick; ref: (u, motion, V, advected at max(Ts)), made here when None.  -> the device's u"""
    want_u, want_m, want_V, want_a = _reference(prev, last, block, radius, echo, max(Ts), scale) if ref is None else ref
    p, l = _dev(prev), _dev(last)
    u, m = ops.trec_flow(p, l, scale, block, radius, echo, return_motion=True)
    assert u.dtype == m.dtype == torch.int32 and tuple(u.shape) == want_u.shape == tuple(m.shape)
    assert (m.cpu().numpy() == want_m).all(), "the integer motion of the same call is not trec_motion's"
    assert torch.equal(ops.trec_flow(p, l, scale, block, radius, echo), u), "the flow depends on whether the motion is asked for"
    got = u.cpu().numpy()
    assert (got == want_u).all(), f"{int((got != want_u).any(axis=-1).sum())} of {got.size // 2} block vectors differ from the refined picks"
    V = ops.flow_field(u, block, *last.shape[-2:])
    assert V.dtype == torch.int32 and tuple(V.shape) == want_V.shape
    assert (V.cpu().numpy() == want_V).all(), f"{int((V.cpu().numpy() != want_V).sum())} of {want_V.size} components of the dense field differ"
    for T in Ts:
        _same_field(ops.advect_flow(l, u, block, T), want_a[:, :T], f"T = {T}")
    return u


# ------------------------------------------------------------------------------------------------ 1. exact against the yardstick
@pytest.mark.parametrize("echo", [1, A.ECHO])
@pytest.mark.parametrize("block,radius", A.CONFIGS, ids=lambda v: str(v))
@pytest.mark.parametrize("case", A.CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_flow_field_and_advection_equal_the_yardstick(case, block, radius, echo):
    """64 x 64 and 128 x 128: whole blocks, 16-byte stores; 33 x 33 and 37 x 53: clipped edge blocks on both axes, float-by-float stores;
    5 x 40: thinner than a block; 16 x 16: one block (or a clipped one)"""
    prev, last = _pair(case)
    ref = _ref(case, block, radius, echo)
    assert (ref[0] != 16 * ref[1]).any(axis=(0, 1, 2)).all(), "the reference refines nothing on one axis: pick another seed"
    assert not np.isnan(ref[3]).any() and len(np.unique(ref[3][:, 5])) > 8
    _check(prev, last, block, radius, echo, (1, 6), ref)


@pytest.mark.parametrize("block,radius", A.CONFIGS, ids=lambda v: str(v))
def test_the_cases_compared_exercise_the_refinement(block, radius):
    print("picks at the edge of the range, invalid blocks of the reference", F.assert_refined(A.CASES, block, radius, fields=_pair))


# ------------------------------------------------------------------------------------------------ 2. values outside the unit range
def test_nan_inf_negatives_and_values_above_one_in_both_frames():
    case = (3, 37, 53, 4)
    prev, last = (a.copy() for a in _pair(case))
    rng = np.random.default_rng(5)
    for a in (prev, last):
        for value in (np.nan, np.inf, -np.inf, -0.75, 1.5, 3.0e38):
            a.reshape(-1)[rng.choice(a.size, 40, replace=False)] = value
    last[0, 8:12, 8:12], prev[0, 8:12, 12:16], prev[1, :4, :4], last[2, -4:, -4:] = np.nan, np.nan, np.nan, np.nan      # whole 4 x 4 patches
    last[1, 0, 0], prev[1, -1, -1], last[2, 36, 0] = np.inf, np.inf, -np.inf
    assert np.isnan(last).sum() > 40 and np.isinf(prev).sum() > 40 and (last < 0).sum() > 40 and (last > 1).sum() > 40
    for block, radius in A.CONFIGS:
        want = _reference(prev, last, block, radius, A.ECHO, 3)
        assert np.isnan(want[3]).any() and np.isinf(want[3]).any() and np.isfinite(want[3]).sum() > want[3].size // 2
        _check(prev, last, block, radius, A.ECHO, (3,), want)
    # zero flow is a copy of every bit pattern, payloads of NaNs included; so is a whole-pixel one
    bits = last.view(np.int32)
    bits[0, 20, 20], bits[0, 20, 21] = 0x7fc01234, np.int32(-0x3fedcc)
    zero = torch.zeros(3, 3, 4, 2, dtype=torch.int32, device=DEV)
    adv = ops.advect_flow(_dev(last), zero, 16, 2).cpu().numpy().view(np.int32)
    assert (adv[:, 0] == bits).all() and (adv[:, 1] == bits).all(), "u = 0 is a copy of every bit pattern"


# ------------------------------------------------------------------------------------------------ 3. the tie to the block scheme
@pytest.mark.parametrize("block,radius", A.CONFIGS, ids=lambda v: str(v))
def test_uniform_whole_pixel_flow_equals_the_block_advection_on_the_device(block, radius):
    for case in ((3, 37, 53, 4), (2, 64, 64, 0)):
        last = _pair(case)[1].copy()
        last[0, 3, 5], last[1, 30, 50], last[0, 0, 0] = np.nan, np.inf, -np.inf
        last.view(np.int32)[0, 20, 20] = 0x7fc01234
        n, H, W = last.shape
        l = _dev(last)
        for v in ((0, 0), (1, -2), (-radius, radius)):
            m = torch.tensor(v, dtype=torch.int32, device=DEV).expand(n, -(-H // block), -(-W // block), 2).contiguous()
            got, want = ops.advect_flow(l, 16 * m, block, 6), ops.advect(l, m, block, 6)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (case, v)
            assert (want.cpu().numpy().view(np.int32) == A.advect(last, m.cpu().numpy(), block, 6).view(np.int32)).all()


# ------------------------------------------------------------------------------------------------ 4. strides and alignment
def _flow_raw(prev_ptr, last_ptr, stride, n, H, W, block, radius, echo, ws=None, u=None, motion=None, scale=SCALE):
    nby, nbx = -(-H // block), -(-W // block)
    nb = lib.query("adnm_trec_flow_ws_bytes", n, H, W, block, radius)
    assert nb == n * nby * nbx * ((2 * radius + 1) ** 2 + 1) * 4
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV) if ws is None else ws
    u = torch.empty((n, nby, nbx, 2), dtype=torch.int32, device=DEV) if u is None else u
    lib.call("adnm_trec_flow", prev_ptr, last_ptr, stride, u.data_ptr(), None if motion is None else motion.data_ptr(), scale, block, radius, echo,
             ws.data_ptr(), nb, n, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return u


def _advect_raw(last_ptr, stride, u, n, T, H, W, block, out=None):
    out = torch.empty((n, T, H, W), dtype=torch.float32, device=DEV) if out is None else out
    lib.call("adnm_advect_flow", last_ptr, stride, u.data_ptr(), out.data_ptr(), block, n, T, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("H,W", [(37, 53), (32, 64)], ids=["odd", "even"])
def test_slices_of_the_input_and_bases_off_by_one_float(H, W):
    B, T_in, T, block, radius = 3, 4, 3, 16, 4
    prev, last = A.two_motion_fields(B, H, W, 1)
    want_u = _check(prev, last, block, radius, A.ECHO, (T,))
    want_a = ops.advect_flow(_dev(last), want_u, block, T)
    assert len({tuple(v) for v in want_u.cpu().numpy().reshape(-1, 2)}) >= 2
    # the two frames as x[:, T_in - 1] and x[:, T_in] of a (B, T_in + 1, H, W) tensor: what the Validator passes
    x = torch.full((B, T_in + 1, H, W), 0.9, dtype=torch.float32, device=DEV)
    x[:, T_in - 1], x[:, T_in] = _dev(prev), _dev(last)
    stride = (T_in + 1) * H * W
    u = _flow_raw(x[:, T_in - 1].data_ptr(), x[:, T_in].data_ptr(), stride, B, H, W, block, radius, A.ECHO)
    assert torch.equal(u, want_u), "slices of a wider tensor"
    a = _advect_raw(x[:, T_in].data_ptr(), stride, u, B, T, H, W, block)
    assert torch.equal(a.view(torch.int32), want_a.view(torch.int32)), "the advected slice"
    # both bases, the flow and the output one float (one int) into a buffer: 4-byte aligned only, so an even W too is stored float by float
    hold = torch.zeros(B * stride + 1, dtype=torch.float32, device=DEV)
    off = hold[1:].view(B, T_in + 1, H, W)
    off.copy_(x)
    assert off[:, T_in].data_ptr() % 16 != x[:, T_in].data_ptr() % 16 and off.data_ptr() % 16 == 4
    hold_u = torch.zeros(want_u.numel() + 1, dtype=torch.int32, device=DEV)
    u = _flow_raw(off[:, T_in - 1].data_ptr(), off[:, T_in].data_ptr(), stride, B, H, W, block, radius, A.ECHO, u=hold_u[1:].view(want_u.shape))
    assert torch.equal(u, want_u) and u.data_ptr() % 8 == 4, "bases one float off the 16-byte boundary"
    out_hold = torch.zeros(B * T * H * W + 1, dtype=torch.float32, device=DEV)
    a = _advect_raw(off[:, T_in].data_ptr(), stride, u, B, T, H, W, block, out=out_hold[1:].view(B, T, H, W))
    assert torch.equal(a.contiguous().view(torch.int32), want_a.view(torch.int32)), "output one float off the 16-byte boundary"


def test_more_blocks_than_the_staged_table_holds():
    """block 8: 64 x 64 = 4096 blocks are staged in LDS, 65 x 65 are read from memory; T = 2 keeps the yardstick short"""
    rng = np.random.default_rng(11)
    for size in (512, 520):
        prev, last = A.two_motion_fields(1, size, size, 3)
        if size == 520:
            _check(prev, last, 8, 2, A.ECHO, (2,))
        # and a flow that differs from block to block, up to the largest a refinement can give
        nb = -(-size // 8)
        u = rng.integers(-136, 137, (1, nb, nb, 2)).astype(np.int32)
        assert (ops.flow_field(_dev(u), 8, size, size).cpu().numpy() == F.field(u, 8, size, size)).all()
        _same_field(ops.advect_flow(_dev(last), _dev(u), 8, 2), F.advect(last, u, 8, 2), f"{nb * nb} blocks")


# ------------------------------------------------------------------------------------------------ 5. workspace contract
@pytest.mark.parametrize("H,W", [(37, 53), (64, 64)], ids=["odd", "even"])
def test_the_workspace_is_fully_written_and_nothing_behind_any_buffer_is(H, W):
    B, T, block, radius, guard = 2, 3, 16, 4, 64
    D = 2 * radius + 1
    nby, nbx = -(-H // block), -(-W // block)
    prev, last = A.two_motion_fields(B, H, W, 1)
    p, l = _dev(prev), _dev(last)
    nb = lib.query("adnm_trec_flow_ws_bytes", B, H, W, block, radius)
    nu, nv, no = B * nby * nbx * 2, B * H * W * 2, B * T * H * W
    results = []
    for fill in (0x00, 0xFF):
        ws = torch.full((nb + guard,), fill, dtype=torch.uint8, device=DEV)
        ws[nb:] = 0xA5
        hold_u, hold_m, hold_v = (torch.full((n + 16,), -7, dtype=torch.int32, device=DEV) for n in (nu, nu, nv))
        hold_o = torch.full((no + 16,), -7.0, dtype=torch.float32, device=DEV)
        u = _flow_raw(p.data_ptr(), l.data_ptr(), H * W, B, H, W, block, radius, A.ECHO, ws=ws, u=hold_u[:nu].view(B, nby, nbx, 2),
                      motion=hold_m[:nu].view(B, nby, nbx, 2))
        V = hold_v[:nv].view(B, H, W, 2)
        lib.call("adnm_flow_field", u.data_ptr(), V.data_ptr(), block, B, H, W, torch.cuda.current_stream().cuda_stream)
        out = _advect_raw(l.data_ptr(), H * W, u, B, T, H, W, block, out=hold_o[:no].view(B, T, H, W))
        assert bool((ws[nb:] == 0xA5).all()), "a write behind ws_bytes"
        assert all(bool((h[n:] == -7).all()) for h, n in ((hold_u, nu), (hold_m, nu), (hold_v, nv), (hold_o, no))), "a write behind flow, motion, field or out"
        # every workspace byte is written: the tables and the echo counts, as the yardstick has them
        tab = ws[:nb].view(torch.int32).view(B, nby, nbx, D * D + 1).cpu().numpy()
        assert (tab[..., :D * D].reshape(B, nby, nbx, D, D) == A.costs(prev, last, SCALE, block, radius)).all()
        assert (tab[..., D * D] == A.echo_counts(last, SCALE, block, A.ECHO)).all()
        results.append((u.clone(), hold_m[:nu].clone(), V.clone(), out.clone()))
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the result depends on what the workspace held"
    want = _reference(prev, last, block, radius, A.ECHO, T)
    assert (results[0][0].cpu().numpy() == want[0]).all() and (results[0][1].view(want[1].shape).cpu().numpy() == want[1]).all()
    assert (results[0][2].cpu().numpy() == want[2]).all()
    _same_field(results[0][3], want[3], "advected")


def test_calls_outside_the_limits_are_refused_and_launch_nothing():
    B, H, W, block, T = 2, 32, 32, 16, 3
    last = torch.rand(B, H, W, device=DEV)
    u = torch.full((B, 2, 2, 2), 16, dtype=torch.int32, device=DEV)
    out = torch.full((B, T, H, W), -7.0, device=DEV)
    V = torch.full((B, H, W, 2), -7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(lib.query("adnm_trec_flow_ws_bytes", B, H, W, block, 4), dtype=torch.uint8, device=DEV)
    so, st = lib.load(), torch.cuda.current_stream().cuda_stream
    flow_out = torch.full_like(u, -7)
    for kw in (dict(T=4097), dict(T=0), dict(block=12), dict(n=0), dict(n=65536), dict(H=32768), dict(stride=H * W - 1)):
        a = dict(dict(T=T, block=block, n=B, H=H, stride=H * W), **kw)
        assert so.adnm_advect_flow(last.data_ptr(), a["stride"], u.data_ptr(), out.data_ptr(), a["block"], a["n"], a["T"], a["H"], W, st) == -1, kw
        assert "advect_flow" in lib.last_error()
    for kw in (dict(block=64), dict(n=0), dict(H=0)):
        a = dict(dict(block=block, n=B, H=H), **kw)
        assert so.adnm_flow_field(u.data_ptr(), V.data_ptr(), a["block"], a["n"], a["H"], W, st) == -1, kw
    for kw in (dict(radius=9), dict(echo=0), dict(scale=256.0), dict(block=4), dict(n=65536)):
        a = dict(dict(radius=4, echo=20, scale=90.0, block=block, n=B), **kw)
        assert so.adnm_trec_flow(last.data_ptr(), last.data_ptr(), H * W, flow_out.data_ptr(), None, a["scale"], a["block"], a["radius"], a["echo"], ws.data_ptr(),
                                 ws.numel(), a["n"], H, W, st) == -1, kw
    assert so.adnm_trec_flow(last.data_ptr(), last.data_ptr(), H * W, flow_out.data_ptr(), None, 90.0, block, 4, 20, ws.data_ptr(), ws.numel() - 1, B, H, W, st) == -3
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((V == -7).all()) and bool((flow_out == -7).all()) and int(ws.sum()) == 0, "a refused call wrote something"
    with pytest.raises(RuntimeError, match="limits"):
        ops.advect_flow(last, u, block, 4097)
    with pytest.raises(RuntimeError, match="int32 tensor"):
        ops.advect_flow(last, u[:, :1], block, T)
    with pytest.raises(RuntimeError, match="int32 tensor"):
        ops.flow_field(u.float(), block, H, W)
    assert so.adnm_advect_flow(last.data_ptr(), H * W, u.data_ptr(), out.data_ptr(), block, B, T, H, W, st) == 0      # and inside them it runs
    torch.cuda.synchronize()
    assert bool((out != -7.0).all())


# ------------------------------------------------------------------------------------------------ 6. the product
def test_extrapolate_is_the_flow_advection_of_the_last_two_frames():
    prev, last = _pair((3, 37, 53, 4))
    x = torch.stack([_dev(prev) * 0.5, _dev(prev), _dev(last)], dim=1)                 # (3, 3, 37, 53)
    want = F.advect(last, F.flow(prev, last, SCALE, 16, 4, 9), 16, 4)
    _same_field(ops.extrapolate(x, 4, SCALE, block=16, radius=4), want, "echo = value_scale / 10")
    _same_field(ops.extrapolate(x[:, :, None], 4, SCALE, 16, 4, echo=9), want, "(n, T_in, 1, H, W)")
    assert tuple(ops.extrapolate(x, 2, SCALE).shape) == (3, 2, 37, 53)
    for bad in (x[:, -1:], x.double(), x[0]):
        with pytest.raises(RuntimeError, match="extrapolate"):
            ops.extrapolate(bad, 4, SCALE)


# ------------------------------------------------------------------------------------------------ 7. the Validator end to end
def test_validator_with_flow_advection_end_to_end():
    import test_advect_gpu as TA
    from adnm_hip.validate import Validator, advection_doubles, block_doubles, fss_doubles
    from models.loss import enRainfallLoss
    model, crit, scale, T = TA._model(), enRainfallLoss(0.57, 0.25, gamma=0.0), 255.0, 20
    pools, scales, n, block, radius = ((4, 4), (16, 8)), (1, 5, 17), len(THR), 16, 4
    base = ((1, 1),) + pools
    host = TA._drifting_samples(4, 7)
    samples = _dev(host)
    data = [(samples[i:i + 2, :5, None].contiguous(), samples[i:i + 2, 5:, None].contiguous()) for i in (0, 2)]
    # the reference first: the yardstick's two advected fields, scored by the pooled and the FSS references
    echo = ops.advection_spec((block, radius), THR)[2]
    ref_u, ref_m = F.flow(host[:, 3], host[:, 4], scale, block, radius, echo, with_parts=True)[:2]
    tgt_all = host[:, 5:].reshape(4 * T, 64, 64)

    def scored(adv):
        a = R.ref_counts(tgt_all, adv.reshape(4 * T, 64, 64), THR, scale, base).reshape(4, T, len(base), -1).sum(0)      # (T, npool, 4 nthr)
        f = FS.ref_sums(tgt_all, adv.reshape(4 * T, 64, 64), THR, scale, scales).reshape(4, T, len(scales), -1).sum(0)
        return a, f
    ref_flow, ref_block = F.advect(host[:, 4], ref_u, block, T), A.advect(host[:, 4], ref_m, block, T)
    assert not np.isnan(ref_flow).any()
    (a_flow, f_flow), (a_block, f_block) = scored(ref_flow), scored(ref_block)
    assert (ref_u != 0).any(axis=(1, 2, 3)).all() and (a_flow[:, 0, 0::4] > 0).all(), "the reference moves or hits nothing: the test is vacuous"
    assert (a_flow != a_block).any() and (f_flow != f_block).any() and (ref_u != 16 * ref_m).any(), "the two schemes cannot be told apart on these inputs"

    val = Validator(model, crit, T, scale, THR, pools=pools, persistence=True, fss=scales, advection=(block, radius), advection_flow=True)
    former = Validator(model, crit, T, scale, THR, pools=pools, persistence=True, fss=scales, advection=(block, radius))
    try:
        def epoch(v):
            for x, tgt in data:
                v.step(x, tgt)
        epoch(val)
        block_bits = val._block.cpu().numpy().copy()
        adv_last, u_last = val.advected(data[1][0]).clone(), val.flow(data[1][0]).clone()
        res, short = val.done(per_lead=True), val.done()
        epoch(former)
        old_block = former._block.cpu().numpy().copy()
        old, old_short = former.done(per_lead=True), former.done()
        # with the flag unset: today's tables and entries, and no new buffer
        at = sum(block_doubles(T, n, pools, True)) + sum(fss_doubles(T, n, scales, True))
        n5, n6 = advection_doubles(T, n, pools, scales, True)
        assert old_block.shape == block_bits.shape == (at + n5 + n6,)
        assert (old_block[at:at + n5].reshape(a_block.shape) == a_block).all() and (old_block[at + n5:].reshape(f_block.shape) == f_block).all()
        assert "scheme" not in old["advection"] and "scheme" not in old_short["advection"]
        assert all(e.get("flow") is None and e["motion"] is not None for e in former._fwd._graphs.values())
        assert all(e["flow"] is not None and e["motion"] is None for e in val._fwd._graphs.values())
        assert (former.advected(data[1][0]).cpu().numpy().view(np.int32) == ref_block[2:4].view(np.int32)).all()
        with pytest.raises(RuntimeError, match="advection_flow"):
            former.flow(data[1][0])
        # the flag moves nothing but the advected field: everything else value for value, the block a bit-exact prefix
        assert set(short) == set(old_short) and set(res["per_lead"]) == set(old["per_lead"])
        assert repr({k: short[k] for k in short if k != "advection"}) == repr({k: old_short[k] for k in short if k != "advection"})
        assert repr({k: res["per_lead"][k] for k in res["per_lead"] if k != "advection"}) == repr({k: old["per_lead"][k] for k in old["per_lead"] if k != "advection"})
        assert (block_bits[:at].view(np.int64) == old_block[:at].view(np.int64)).all(), "the tables in front of the advection's moved"
        # the two tables of the advected field, integer for integer
        got_a, got_f = block_bits[at:at + n5].reshape(a_flow.shape), block_bits[at + n5:].reshape(f_flow.shape)
        assert (got_a == a_flow).all(), f"{int((got_a != a_flow).sum())} of {a_flow.size} pooled counts of the advected field differ"
        assert (got_f == f_flow).all(), f"{int((got_f != f_flow).sum())} of {f_flow.size} FSS sums of the advected field differ"
        # the scores
        adv, lead = res["advection"], res["per_lead"]["advection"]
        assert set(adv) == {"threshold_metrics", "FAR", "pooled", "fss", "scheme"} and adv["scheme"] == short["advection"]["scheme"] == "flow"
        assert set(lead) == {"threshold_metrics", "pooled", "fss"}
        TA._check_scored(adv, lead, a_flow[:, 0], "flow advection")
        for i, p in enumerate(base[1:], start=1):
            TA._check_scored(adv["pooled"][p], lead["pooled"][p], a_flow[:, i], f"flow advection pooled {p}")
        total, per = FS.fss(f_flow.sum(axis=0)), FS.fss(f_flow)
        for i, s in enumerate(scales):
            for k, thr in enumerate(THR):
                assert TA._close(adv["fss"][s][thr], total[i, k]) and TA._close(lead["fss"][s][thr], per[:, i, k]), (s, thr)
        # advected() and flow(): the static tensors of the last batch of that shape
        assert (u_last.cpu().numpy() == ref_u[2:4]).all()
        _same_field(adv_last, ref_flow[2:4], "advected()")
        assert torch.equal(adv_last.view(torch.int32), ops.extrapolate(samples[2:4, :5], T, scale, block, radius, echo).view(torch.int32))
        # a second epoch replays the graph: the same bits; and a step allocates nothing
        val.done(reset=True)
        epoch(val)
        assert (val._block.cpu().numpy().view(np.int64) == block_bits.view(np.int64)).all()
        assert repr(val.done(reset=True, per_lead=True)) == repr(res)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        val.step(*data[0])
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    finally:
        val.close()
        former.close()
