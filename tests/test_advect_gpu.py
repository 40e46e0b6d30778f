"""Block-matched motion and advection on the GPU (csrc/advect.hip: adnm_trec_motion, adnm_advect; ops.trec_motion, ops.advect;
Validator(advection=)): exact, integer for integer and bit for bit, against the CPU yardstick (advect_ref), at every addressing the
Validator uses, and end to end through the captured graph.  The floats derived from the summed counts use the same double expression
on both sides and are compared to 1e-12 relative."""
import numpy as np
import pytest
import torch

import advect_ref as A
import fss_ref as F
import verify_ref as R
from adnm_hip import lib, ops, recipe

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


def _ref(case, block, radius, echo):
    """the CPU reference (motion, costs) of a case, made once and never written to"""
    key = (case, block, radius, echo)
    if key not in _refs:
        prev, last = _pair(case)
        _refs[key] = A.motion(prev, last, SCALE, block, radius, echo, with_parts=True)[:2]
        for a in _refs[key]:
            a.setflags(write=False)
    return _refs[key]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the cached fields are read-only)


def _check_motion(prev, last, block, radius, echo, ref=None, scale=SCALE):
    m, c = ops.trec_motion(_dev(prev), _dev(last), scale, block, radius, echo, return_costs=True)
    want_m, want_c = A.motion(prev, last, scale, block, radius, echo, with_parts=True)[:2] if ref is None else ref
    assert m.dtype == c.dtype == torch.int32 and tuple(m.shape) == want_m.shape and tuple(c.shape) == want_c.shape
    m, c = m.cpu().numpy(), c.cpu().numpy().astype(np.int64)
    assert (c == want_c).all(), f"{int((c != want_c).sum())} of {c.size} costs differ from the sums of absolute differences on the quantised frames"
    assert (m == want_m).all(), f"{int((m != want_m).any(axis=-1).sum())} of {m.size // 2} vectors differ from the pick of the (equal) cost tables"
    return m


def _check_advect(last, m, block, T):
    got = ops.advect(_dev(last), _dev(m), block, T)
    want = A.advect(last, m, block, T)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    got = got.cpu().numpy().view(np.int32)
    assert (got == want.view(np.int32)).all(), f"{int((got != want.view(np.int32)).sum())} of {got.size} cells differ from the gathered bit patterns"


# ------------------------------------------------------------------------------------------------ 1. exact against the yardstick
@pytest.mark.parametrize("echo", [1, A.ECHO])
@pytest.mark.parametrize("block,radius", A.CONFIGS, ids=lambda v: str(v))
@pytest.mark.parametrize("case", A.CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_costs_vectors_and_advection_equal_the_yardstick(case, block, radius, echo):
    """64 x 64 and 128 x 128: whole blocks, 16-byte loads; 33 x 33 and 37 x 53: clipped edge blocks on both axes, float-by-float loads;
    5 x 40: thinner than a block; 16 x 16: one block (or a clipped one)"""
    prev, last = _pair(case)
    ref = _ref(case, block, radius, echo)
    assert len({tuple(v) for v in ref[0].reshape(-1, 2)}) >= 2 and (ref[0] != 0).any(axis=(1, 2, 3)).all(), "the reference moves nothing: pick another seed"
    m = _check_motion(prev, last, block, radius, echo, ref)
    _check_advect(last, m, block, 5)


@pytest.mark.parametrize("block,radius", A.CONFIGS, ids=lambda v: str(v))
def test_the_cases_compared_are_dense(block, radius):
    print("tied, invalid blocks of the reference", A.assert_dense(A.CASES, block, radius, fields=_pair))


# ------------------------------------------------------------------------------------------------ 2. non-finite input
def test_nan_quantises_to_zero_and_the_advected_field_keeps_every_bit_pattern():
    case = (3, 37, 53, 4)
    prev, last = (a.copy() for a in _pair(case))
    rng = np.random.default_rng(5)
    for a in (prev, last):
        for value in (np.nan, np.inf, -np.inf):
            a.reshape(-1)[rng.choice(a.size, 40, replace=False)] = value
    last[0, 8:12, 8:12], prev[0, 8:12, 12:16], prev[1, :4, :4], last[2, -4:, -4:] = np.nan, np.nan, np.nan, np.nan      # whole 4 x 4 patches
    last[1, 0, 0], prev[1, -1, -1], last[2, 36, 0] = np.inf, np.inf, -np.inf
    bits = last.view(np.int32)
    bits[0, 20, 20], bits[0, 20, 21] = 0x7fc01234, np.int32(-0x3fedcc)          # NaNs with payloads, quiet and negative
    assert np.isnan(last).sum() > 60 and np.isinf(prev).sum() > 40
    for block, radius in A.CONFIGS:
        m = _check_motion(prev, last, block, radius, A.ECHO)
        _check_advect(last, m, block, 3)
    adv = ops.advect(_dev(last), torch.zeros(3, 3, 4, 2, dtype=torch.int32, device=DEV), 16, 2).cpu().numpy().view(np.int32)
    assert (adv[:, 0] == bits).all() and (adv[:, 1] == bits).all(), "v = 0 is a copy of every bit pattern"


# ------------------------------------------------------------------------------------------------ 3. strides and alignment
def _motion_raw(prev_ptr, last_ptr, stride, n, H, W, block, radius, echo, ws=None, motion=None, costs=None, scale=SCALE):
    D = 2 * radius + 1
    nby, nbx = -(-H // block), -(-W // block)
    nb = lib.query("adnm_trec_ws_bytes", n, H, W, block, radius)
    assert nb == n * nby * nbx * (D * D + 1) * 4
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV) if ws is None else ws
    motion = torch.empty((n, nby, nbx, 2), dtype=torch.int32, device=DEV) if motion is None else motion
    costs = torch.empty((n, nby, nbx, D, D), dtype=torch.int32, device=DEV) if costs is None else costs
    lib.call("adnm_trec_motion", prev_ptr, last_ptr, stride, motion.data_ptr(), costs.data_ptr(), scale, block, radius, echo, ws.data_ptr(), nb, n, H, W,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return motion, costs


def _advect_raw(last_ptr, stride, motion, n, T, H, W, block, out=None):
    out = torch.empty((n, T, H, W), dtype=torch.float32, device=DEV) if out is None else out
    lib.call("adnm_advect", last_ptr, stride, motion.data_ptr(), out.data_ptr(), block, n, T, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("H,W", [(37, 53), (32, 64)], ids=["odd", "even"])
def test_slices_of_the_input_and_bases_off_by_one_float(H, W):
    B, T_in, T, block, radius = 3, 4, 3, 16, 4
    prev, last = A.two_motion_fields(B, H, W, 1)
    want_m, want_c = ops.trec_motion(_dev(prev), _dev(last), SCALE, block, radius, A.ECHO, return_costs=True)
    want_a = ops.advect(_dev(last), want_m, block, T)
    ref_m, ref_c = A.motion(prev, last, SCALE, block, radius, A.ECHO, with_parts=True)[:2]
    assert (want_m.cpu().numpy() == ref_m).all() and (want_c.cpu().numpy() == ref_c).all() and len({tuple(v) for v in ref_m.reshape(-1, 2)}) >= 2
    # the two frames as x[:, T_in - 1] and x[:, T_in] of a (B, T_in + 1, H, W) tensor: what the Validator passes
    x = torch.full((B, T_in + 1, H, W), 0.9, dtype=torch.float32, device=DEV)
    x[:, T_in - 1], x[:, T_in] = _dev(prev), _dev(last)
    stride = (T_in + 1) * H * W
    m, c = _motion_raw(x[:, T_in - 1].data_ptr(), x[:, T_in].data_ptr(), stride, B, H, W, block, radius, A.ECHO)
    assert torch.equal(m, want_m) and torch.equal(c, want_c), "slices of a wider tensor"
    a = _advect_raw(x[:, T_in].data_ptr(), stride, m, B, T, H, W, block)
    assert torch.equal(a.view(torch.int32), want_a.view(torch.int32)), "the advected slice"
    # both bases (and the output) one float into a buffer: 4-byte aligned only, so an even W too is read and stored float by float
    hold = torch.zeros(B * stride + 1, dtype=torch.float32, device=DEV)
    off = hold[1:].view(B, T_in + 1, H, W)
    off.copy_(x)
    assert off[:, T_in].data_ptr() % 16 != x[:, T_in].data_ptr() % 16 and off.data_ptr() % 16 == 4
    m, c = _motion_raw(off[:, T_in - 1].data_ptr(), off[:, T_in].data_ptr(), stride, B, H, W, block, radius, A.ECHO)
    assert torch.equal(m, want_m) and torch.equal(c, want_c), "bases one float off the 16-byte boundary"
    out_hold = torch.zeros(B * T * H * W + 1, dtype=torch.float32, device=DEV)
    a = _advect_raw(off[:, T_in].data_ptr(), stride, m, B, T, H, W, block, out=out_hold[1:].view(B, T, H, W))
    assert torch.equal(a.contiguous().view(torch.int32), want_a.view(torch.int32)), "output one float off the 16-byte boundary"


# ------------------------------------------------------------------------------------------------ 4. workspace contract
@pytest.mark.parametrize("H,W", [(37, 53), (64, 64)], ids=["odd", "even"])
def test_the_workspace_is_fully_written_and_nothing_behind_any_buffer_is(H, W):
    B, T, block, radius, guard = 2, 3, 16, 4, 64
    D = 2 * radius + 1
    nby, nbx = -(-H // block), -(-W // block)
    prev, last = A.two_motion_fields(B, H, W, 1)
    p, l = _dev(prev), _dev(last)
    nb = lib.query("adnm_trec_ws_bytes", B, H, W, block, radius)
    nm, nc, no = B * nby * nbx * 2, B * nby * nbx * D * D, B * T * H * W
    results = []
    for fill in (0x00, 0xFF):
        ws = torch.full((nb + guard,), fill, dtype=torch.uint8, device=DEV)
        ws[nb:] = 0xA5
        hold_m, hold_c = (torch.full((n + 16,), -7, dtype=torch.int32, device=DEV) for n in (nm, nc))
        hold_o = torch.full((no + 16,), -7.0, dtype=torch.float32, device=DEV)
        m, c = _motion_raw(p.data_ptr(), l.data_ptr(), H * W, B, H, W, block, radius, A.ECHO, ws=ws, motion=hold_m[:nm].view(B, nby, nbx, 2),
                           costs=hold_c[:nc].view(B, nby, nbx, D, D))
        out = _advect_raw(l.data_ptr(), H * W, m, B, T, H, W, block, out=hold_o[:no].view(B, T, H, W))
        assert bool((ws[nb:] == 0xA5).all()), "a write behind ws_bytes"
        assert bool((hold_m[nm:] == -7).all()) and bool((hold_c[nc:] == -7).all()) and bool((hold_o[no:] == -7.0).all()), "a write behind motion, cost_out or out"
        # every workspace byte is written: the tables and the echo counts, as the yardstick has them
        tab = ws[:nb].view(torch.int32).view(B, nby, nbx, D * D + 1).cpu().numpy()
        assert (tab[..., :D * D].reshape(B, nby, nbx, D, D) == A.costs(prev, last, SCALE, block, radius)).all()
        assert (tab[..., D * D] == A.echo_counts(last, SCALE, block, A.ECHO)).all()
        results.append((m.clone(), c.clone(), out.clone()))
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "the result depends on what the workspace held"
    assert (results[0][0].cpu().numpy() == A.motion(prev, last, SCALE, block, radius, A.ECHO)).all()


# ------------------------------------------------------------------------------------------------ 5. the tie rule
def test_ties_fall_towards_zero_in_the_prescribed_order():
    zero = torch.zeros(2, 40, 40, device=DEV)
    for block, radius in A.CONFIGS:
        m, c = ops.trec_motion(zero, zero, SCALE, block, radius, 1, return_costs=True)
        assert int(m.abs().sum()) == 0 and int(c.abs().sum()) == 0, "two empty frames"
    # prev: two equal points at (10, 8) and (10, 12); last: one at (10, 10).  (dy, dx) = (0, 2) and (0, -2) cost the same (one unmatched
    # point each), every other displacement more: the order takes the smaller dx
    prev, last = np.zeros((1, 32, 32), dtype=np.float32), np.zeros((1, 32, 32), dtype=np.float32)
    prev[0, 10, 8] = prev[0, 10, 12] = last[0, 10, 10] = 0.5
    m, c, valid, g = A.motion(prev, last, SCALE, 32, 4, 1, with_parts=True)
    assert c[0, 0, 0, 4, 6] == c[0, 0, 0, 4, 2] == 45 == c.min() and (c == 45).sum() == 2 and tuple(m[0, 0, 0]) == (0, -2) and not valid.any()
    assert (_check_motion(prev, last, 32, 4, 1)[0, 0, 0] == (0, -2)).all()
    # the same pair turned by 90 degrees: (2, 0) and (-2, 0) tie, the smaller dy wins
    assert (_check_motion(prev.transpose(0, 2, 1).copy(), last.transpose(0, 2, 1).copy(), 32, 4, 1)[0, 0, 0] == (-2, 0)).all()
    # a diagonal and an axial candidate of equal cost: the shorter vector wins, (0, 2) over (-2, -2)
    prev[:] = 0
    prev[0, 10, 8], prev[0, 12, 12] = 0.5, 0.5
    m = _check_motion(prev, last, 32, 4, 1)
    assert (m[0, 0, 0] == (0, 2)).all()
    # a valid block (32 echo pixels) takes its own pick, here against a different global vector
    prev, last = np.zeros((1, 16, 48), dtype=np.float32), np.zeros((1, 16, 48), dtype=np.float32)
    last[0, 4:8, 4:12], prev[0, 4:8, 5:13] = 0.5, 0.5                                  # block 0: 32 pixels, moved by (0, -1)
    last[0, 2:5, 20:23], prev[0, 4:7, 20:23] = 0.9, 0.9                                # block 1: 9 brighter pixels, moved by (-2, 0): not valid
    last[0, 2:5, 36:39], prev[0, 4:7, 36:39] = 0.9, 0.9                                # block 2: the same
    m, c, valid, g = A.motion(prev, last, SCALE, 16, 2, 1, with_parts=True)
    assert valid.tolist() == [[[True, False, False]]] and tuple(g[0]) == (-2, 0) and m[0, 0].tolist() == [[0, -1], [-2, 0], [-2, 0]]
    _check_motion(prev, last, 16, 2, 1)


# ------------------------------------------------------------------------------------------------ 6. the Validator end to end
def _model():
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(m)
    return m.to(DEV).eval()


def _drifting_samples(n, seed):
    """test_fss_gpu's: frame j of a sample is its blob field moved j pixels along x, scaled into the radar range"""
    rng = np.random.default_rng(seed)
    base = 0.45 * R.blobs(rng, n, 64, 64, 3) + rng.normal(0.0, 0.004, size=(n, 64, 64))
    return np.stack([np.roll(base, j, axis=2) for j in range(25)], axis=1).astype(np.float32)


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= 1e-12 * np.abs(b))).all())


def _csi(rows):
    """(..., 4 * nthr) TP, FN, FP, TN -> (..., nthr)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return rows[..., 0::4] / (rows[..., 0::4] + rows[..., 1::4] + rows[..., 2::4])


def _check_scored(got, lead, rows, what):
    """got / lead: the entries of a scored field; rows: (T, 4 * nthr) reference counts"""
    from adnm_hip.evaluator import contingency_metrics
    want, far = contingency_metrics(rows.sum(axis=0), THR)
    assert list(got["threshold_metrics"]) == THR
    for k, thr in enumerate(THR):
        for name in ("TP", "FN", "FP", "TN"):
            assert got["threshold_metrics"][thr][name] == want[thr][name], (what, thr, name)
            assert (lead["threshold_metrics"][thr][name] == rows[:, 4 * k + ("TP", "FN", "FP", "TN").index(name)]).all(), (what, "per lead", thr, name)
        for name in ("CSI", "POD", "HSS"):
            assert _close(got["threshold_metrics"][thr][name], want[thr][name]), (what, thr, name)
        assert _close(lead["threshold_metrics"][thr]["CSI"], _csi(rows)[:, k]), (what, "per lead CSI", thr)
    assert _close(got["FAR"], float(np.mean(far))), what


def test_validator_with_advection_pools_persistence_and_fss_end_to_end():
    from adnm_hip.dataio import ResidentDataset
    from adnm_hip.validate import Validator, advection_doubles, block_doubles, fss_doubles
    from models.loss import enRainfallLoss
    model, crit, scale, T = _model(), enRainfallLoss(0.57, 0.25, gamma=0.0), 255.0, 20
    pools, scales, n, block, radius = ((4, 4), (16, 8)), (1, 5, 17), len(THR), 16, 4
    base = ((1, 1),) + pools
    host = _drifting_samples(6, 7)
    samples = _dev(host)
    data = [(samples[i:i + 2, :5, None].contiguous(), samples[i:i + 2, 5:, None].contiguous()) for i in (0, 2, 4)]
    feed = ResidentDataset.from_frames(samples[4:6].contiguous(), 5, 2, DEV, shuffle=False)
    # the reference first: the yardstick's advected field, scored by the pooled and the FSS references
    echo = ops.advection_spec((block, radius), THR)[2]
    assert echo == 10
    ref_m = A.motion(host[:, 3], host[:, 4], scale, block, radius, echo)
    ref_adv = A.advect(host[:, 4], ref_m, block, T)                                                # (6, T, 64, 64)
    tgt_all = host[:, 5:].reshape(6 * T, 64, 64)
    held = np.broadcast_to(host[:, 4:5], (6, T, 64, 64)).reshape(6 * T, 64, 64)
    a_ref = R.ref_counts(tgt_all, ref_adv.reshape(6 * T, 64, 64), THR, scale, base).reshape(6, T, len(base), -1).sum(0)      # (T, npool, 4 nthr)
    b_ref = R.ref_counts(tgt_all, held, THR, scale, base).reshape(6, T, len(base), -1).sum(0)
    af_ref = F.ref_sums(tgt_all, ref_adv.reshape(6 * T, 64, 64), THR, scale, scales).reshape(6, T, len(scales), -1).sum(0)
    # on these inputs the advection beats holding the frame at every threshold and frame index: asserted on the REFERENCE, so that a
    # change of the inputs cannot hide behind the kernel
    csi_a, csi_b = _csi(a_ref[:, 0]), _csi(b_ref[:, 0])
    print("advection CSI, smallest per threshold", csi_a.min(axis=0), "persistence CSI, largest per threshold", csi_b.max(axis=0))
    assert (csi_a > csi_b).all(), "the reference's advection does not beat its persistence: the inputs changed"
    assert (ref_m != 0).any(axis=(1, 2, 3)).all() and (a_ref[:, 0, 0::4] > 0).all(), "the reference moves or hits nothing: the test is vacuous"

    val = Validator(model, crit, T, scale, THR, pools=pools, persistence=True, fss=scales, advection=(block, radius))
    former = Validator(model, crit, T, scale, THR, pools=pools, persistence=True, fss=scales)
    try:
        def epoch(v):
            feed.begin_epoch()
            for x, tgt in data[:2]:
                v.step(x, tgt)
            v.step_from(feed)                                   # the third batch straight into the graph's static buffers
        epoch(val)
        block_bits = val._block.cpu().numpy().copy()
        adv_last = val.advected(data[2][0]).clone()
        res, short = val.done(per_lead=True), val.done()
        epoch(former)
        old_block = former._block.cpu().numpy().copy()
        old, old_short = former.done(per_lead=True), former.done(reset=True)
        # nothing that was there moved: the shared keys value for value, the block a bit-exact prefix
        assert set(short) == set(old_short) | {"advection"} and set(res["per_lead"]) == set(old["per_lead"]) | {"advection"}
        assert repr({k: short[k] for k in old_short}) == repr(old_short)
        assert repr({k: res[k] for k in old if k != "per_lead"}) == repr({k: old[k] for k in old if k != "per_lead"})
        assert repr({k: res["per_lead"][k] for k in old["per_lead"]}) == repr(old["per_lead"])
        at = sum(block_doubles(T, n, pools, True)) + sum(fss_doubles(T, n, scales, True))
        n5, n6 = advection_doubles(T, n, pools, scales, True)
        assert old_block.shape == (at,) and block_bits.shape == (at + n5 + n6,)
        assert (block_bits[:at].view(np.int64) == old_block.view(np.int64)).all(), "the former block is not a bit-exact prefix"
        # the two appended tables, integer for integer
        got_a, got_f = block_bits[at:at + n5].reshape(a_ref.shape), block_bits[at + n5:].reshape(af_ref.shape)
        assert (got_a == a_ref).all(), f"{int((got_a != a_ref).sum())} of {a_ref.size} pooled counts of the advected field differ"
        assert (got_f == af_ref).all(), f"{int((got_f != af_ref).sum())} of {af_ref.size} FSS sums of the advected field differ"
        # the scores
        adv, lead = res["advection"], res["per_lead"]["advection"]
        assert set(adv) == {"threshold_metrics", "FAR", "pooled", "fss"} and set(lead) == {"threshold_metrics", "pooled", "fss"}
        _check_scored(adv, lead, a_ref[:, 0], "advection")
        for i, p in enumerate(base[1:], start=1):
            _check_scored(adv["pooled"][p], lead["pooled"][p], a_ref[:, i], f"advection pooled {p}")
        total, per = F.fss(af_ref.sum(axis=0)), F.fss(af_ref)
        for i, s in enumerate(scales):
            for k, thr in enumerate(THR):
                assert _close(adv["fss"][s][thr], total[i, k]) and _close(lead["fss"][s][thr], per[:, i, k]), (s, thr)
        for k, thr in enumerate(THR):
            assert (lead["threshold_metrics"][thr]["CSI"] > res["per_lead"]["persistence"]["threshold_metrics"][thr]["CSI"]).all(), thr
            assert adv["threshold_metrics"][thr]["CSI"] > res["persistence"]["threshold_metrics"][thr]["CSI"]
        # advected(): the static forecast of the last batch of that shape
        want = ops.advect(samples[4:6, 4], ops.trec_motion(samples[4:6, 3], samples[4:6, 4], scale, block, radius, echo), block, T)
        assert torch.equal(adv_last.view(torch.int32), want.view(torch.int32)) and (want.cpu().numpy().view(np.int32) == ref_adv[4:6].view(np.int32)).all()
        # a second epoch replays the graph: the same bits; and a step allocates nothing
        val.done(reset=True)
        assert float(val._block.abs().sum()) == 0.0, "done(reset=True) left something in the block or the tables"
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


def test_validator_with_advection_alone_and_the_plain_validator_allocates_nothing_new():
    from adnm_hip.validate import Validator, block_doubles
    from models.loss import RainfallLoss

    class LastFrames(torch.nn.Module):
        def forward(self, x):
            return x[:, -1:, 0].float().expand(-1, 20, -1, -1) * 0.9

    host = _drifting_samples(2, 3)
    frames = _dev(host)[:, :, None].contiguous()
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    val = Validator(LastFrames(), RainfallLoss(), 20, 255.0, THR, advection=True)
    plain = Validator(LastFrames(), RainfallLoss(), 20, 255.0, THR)
    try:
        val.step(x, tgt)
        plain.step(x, tgt)
        assert plain._block.numel() == block_doubles(20, len(THR))[0] and val._block.numel() == plain._block.numel() + 20 * 4 * len(THR)
        assert all(e.get("adv") is None and e.get("ws_trec") is None and e.get("motion") is None and e.get("ws_pool") is None for e in plain._fwd._graphs.values())
        res, old = val.done(per_lead=True), plain.done(per_lead=True)
        assert set(res) == set(old) | {"advection"} and repr({k: res[k] for k in old if k != "per_lead"}) == repr({k: old[k] for k in old if k != "per_lead"})
        m = A.motion(host[:, 3], host[:, 4], 255.0, 32, 4, 10)
        want = R.ref_counts(host[:, 5:].reshape(40, 64, 64), A.advect(host[:, 4], m, 32, 20).reshape(40, 64, 64), THR, 255.0, [(1, 1)]).reshape(2, 20, -1).sum(0)
        _check_scored(res["advection"], res["per_lead"]["advection"], want, "advection alone")
        assert res["advection"]["pooled"] == {} and "fss" not in res["advection"]
        with pytest.raises(RuntimeError, match="advected"):
            plain.advected(x)
    finally:
        val.close()
        plain.close()
    one = Validator(LastFrames(), RainfallLoss(), 20, 255.0, THR, advection=True)
    try:
        with pytest.raises(RuntimeError, match="last two input frames"):
            one.step(x[:, -1:].contiguous(), tgt)
    finally:
        one.close()


# ------------------------------------------------------------------------------------------------ 7. fp8 mode
def test_a_validation_epoch_with_advection_leaves_the_fp8_table_alone():
    import test_validate_gpu as V
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    data = V._batches()
    with V._Precision("fp8"):
        model = V._model()
        tr = V._trainer(model)
        val = Validator(model, enRainfallLoss(0.57, 0.25, gamma=0.0), 20, 255.0, THR, advection=True)
        try:
            tr.step(*data[0])
            tr.step(*data[1])            # period 2: the record flags are set while the validation epoch runs
            torch.cuda.synchronize()
            dev = next(model.parameters()).device
            table = ops.QUANT.table(dev).clone()
            assert bool((table[:, :2] != 1.0).any()), "no record ever made a scale: nothing is tested"
            for x, tgt in data[3:5]:
                val.step(x, tgt)
            res = val.done(reset=True)
            after = ops.QUANT.table(dev)
            assert torch.equal(table.view(torch.int32), after.view(torch.int32)), "the validation epoch wrote into the delayed-scaling table"
            assert res["batches"] == 2 and res["nonfinite"] == 0 and "advection" in res
            tr.step(*data[2])
        finally:
            val.close()
            tr.close()
