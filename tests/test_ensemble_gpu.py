"""The ensemble on the device (csrc/ensemble.hip) against the CPU yardstick (ensemble_ref): the symmetries of the square and their undoing bit
for bit, adnm_valid_ens_accum's table integer for integer on every tail, path and degenerate stack, adnm_ensemble_product bit for bit, and
the Validator and the Forecaster through their captured graphs around stand-in models whose members the CPU can restate exactly; once the
real model."""
import ctypes

import numpy as np
import pytest
import torch

import ensemble_ref as E
from adnm_hip import lib, ops
from adnm_hip import validate as V
from util import guarded_workspaces, poisoned_outputs, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = 90.0
THRS = {1: [35.0], 4: [20.0, 30.0, 35.0, 40.0], 5: [0.0, 1.0, 35.0, 89.5, 90.0], 8: [5.0, 10.0, 20.0, 30.0, 35.0, 40.0, 60.0, 91.0]}
PAIRS = [(2, 1), (3, 4), (8, 5), (16, 8)]     # (M, thresholds)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the symmetries
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 5), (31, 31), (32, 32), (33, 33), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_members_and_their_undoing_equal_the_torch_yardstick_bit_for_bit(shape):
    H, W = shape
    codes = list(range(8)) if H == W else [0, 1, 2, 3]
    codes = codes + [codes[-1], 0]      # a code twice: the members need not be distinct here
    rng = np.random.default_rng(H * 100 + W)
    x = rng.normal(size=(2, 3, H, W)).astype(np.float32)
    flat = x.reshape(-1).view(np.uint32)
    for k, pattern in enumerate((0x7FC12345, 0xFFC00001, 0x80000000, 0x7F800000, 0x00000001)):     # NaN payloads, -0.0, +Inf, a denormal
        flat[(k * 37) % flat.size] = pattern
    xd = _dev(x)
    fwd = ops.d4_members(xd, codes)
    assert fwd.shape == (len(codes), 2, 3, H, W) and torch.equal(_bits(fwd).cpu(), _bits(E.members(torch.from_numpy(x), codes))), "forward"
    stack = rng.normal(size=(len(codes), 2, 3, H, W)).astype(np.float32)
    stack.reshape(-1).view(np.uint32)[::41] = 0x7FC54321
    inv = ops.d4_members(_dev(stack), codes, inverse=True)
    assert torch.equal(_bits(inv).cpu(), _bits(E.members(torch.from_numpy(stack), codes, inverse=True))), "inverse"
    back = ops.d4_members(fwd, codes, inverse=True)
    assert all(torch.equal(_bits(back[m]), _bits(xd)) for m in range(len(codes))), "inverse(forward(x)) is x"
    # a 4-byte aligned slice on both sides: float by float, the same result
    hold_in, hold_out = torch.zeros(x.size + 1, device=DEV), torch.full((len(codes) * x.size + 3,), -7.0, device=DEV)
    src, dst = hold_in[1:].view(xd.shape), hold_out[1:-2].view(fwd.shape)
    src.copy_(xd)
    assert src.data_ptr() % 16 == 4 and dst.data_ptr() % 16 == 4
    ops.d4_members_into(src, dst, (ctypes.c_int * len(codes))(*codes), len(codes), False)
    assert torch.equal(_bits(dst), _bits(fwd)) and float(hold_out[0]) == -7.0 and bool((hold_out[-2:] == -7.0).all()), "the misaligned slice, and what lies round it"


def test_every_element_is_written_and_a_transposing_code_on_other_frames_raises(monkeypatch):
    for shape, codes in (((2, 33, 33), range(8)), ((3, 8, 12), range(4)), ((1, 64, 64), (0, 5, 6))):
        x = torch.rand(shape, device=DEV)
        recs = []
        for pattern in (0, 1):
            with poisoned_outputs(monkeypatch, pattern) as p:
                ops.d4_members(x, list(codes))
                ops.d4_members(ops.d4_members(x, list(codes)), list(codes), inverse=True)
                torch.cuda.synchronize()
                recs.append(p.records)
        assert len(recs[0]) == 3 and unwritten(*recs) == {}, shape
    for code in (4, 5, 6, 7):
        with pytest.raises(ValueError, match="square"):
            ops.d4_members(torch.zeros(2, 8, 12, device=DEV), [0, code])
        with pytest.raises(RuntimeError, match="square"):
            ops.d4_members_into(torch.zeros(2, 8, 12, device=DEV), torch.zeros(2, 2, 8, 12, device=DEV), (ctypes.c_int * 2)(0, code), 2, False)
    with pytest.raises(ValueError):
        ops.d4_members(torch.zeros(2, 8, 8, device=DEV), [0, 8])


# ------------------------------------------------------------------------------------------------ 2. the score
def _check(t, m, thr, scale=SCALE, what=""):
    got = ops.ensemble_table(_dev(t), _dev(m), thr, scale)
    ref = E.frame_rows(t, m, thr, scale)
    assert got.dtype == torch.int64 and got.shape == ref.shape
    same = got.cpu().numpy() == ref
    assert same.all(), f"{what}: first difference at (frame, column) {np.argwhere(~same)[0].tolist()}: {got.cpu().numpy()[~same][0]} vs {ref[~same][0]}"
    return ref


@pytest.mark.parametrize("hw", [1, 7, 63, 64, 65, 4095, 4096, 4097])
def test_the_table_equals_the_yardstick_round_the_wave_the_quad_and_the_item(hw):
    for M, n in PAIRS:
        t, m = E.radar_stack(M, 3, 1, hw, hw + M)
        ref = _check(t, m, THRS[n], what=f"hw {hw} M {M}")
        assert (ref[:, 0] == hw).all()
    t, m = E.noise_stack(8, 2, 1, hw, hw)
    _check(t, m, THRS[4], what=f"noise hw {hw}")


def test_the_table_equals_the_yardstick_on_radar_like_frames_of_128_x_128():
    for M, n in PAIRS:
        t, m = E.radar_stack(M, 2, 128, 128, 40 + M)
        ref = _check(t, m, THRS[n], what=f"128 x 128 M {M}")
        assert (ref[:, 1] > 0.7 * 128 * 128).all() and (ref[:, 4] > 0).all() and (ref[:, 7:].sum(axis=1) > 0).all(), "mostly dry, and yet something to compare"


@pytest.mark.parametrize("scale", [1.0, 90.0, 255.0, 90.7])
def test_degenerate_stacks_and_value_scales(scale):
    H, W, thr = 37, 45, [t for t in THRS[5] if t <= scale] + [scale + 1.0]
    for M in (2, 8, 16):
        Q, C = int(np.floor(scale)), E.cols(M, len(thr))
        zeros = np.zeros((2, H, W), dtype=np.float32)
        ref = _check(zeros, np.zeros((M, 2, H, W), dtype=np.float32), thr, scale, "all zero")
        assert (ref[:, :2] == H * W).all() and (ref[:, 2:] == 0).all() and ref.shape == (2, C), "only N and Z move"
        ones = np.full((2, H, W), 3.0, dtype=np.float32)
        ref = _check(ones, np.full((M, 2, H, W), np.inf, dtype=np.float32), thr, scale, "all Q")
        assert (ref[:, 1:7] == 0).all() and (ref[:, 7 + M] == H * W).all(), "every member equals the target: rank bin (0, M)"
        t, m = E.radar_stack(M, 2, H, W, 3)
        ref = _check(t, np.broadcast_to(t, (M,) + t.shape).copy(), thr, scale, "members equal to the target")
        assert (ref[:, 2:7] == 0).all()
        ref = _check(t, np.broadcast_to(m[1], m.shape).copy(), thr, scale, "M copies of one field")
        assert (ref[:, 4:6] == 0).all() and (ref[:, 3] == M * ref[:, 2]).all()
        tn, mn = E.noise_stack(M, 2, H, W, 5)
        ref = _check(tn, mn, thr, scale, "uniform noise")
        assert Q > 1 or (ref[:, 1] > 0).all()


def _table(T, M, nthr, fill=0.0):
    n = lib.query("adnm_valid_ens_block_bytes", T, nthr, M) // 8
    assert n == T * E.cols(M, nthr)
    return torch.full((n,), fill, dtype=torch.float64, device=DEV)


def _accum(mem, ms, ss, fs, tgt, table, thr, M, T, hw):
    frames = tgt.numel() // hw
    assert lib.query("adnm_valid_ens_accum_ws_bytes", frames, T, hw, len(thr), M, SCALE) == 0
    ops.ensemble_accum_into(mem, ms, ss, fs, tgt, table, (ctypes.c_float * len(thr))(*thr), len(thr), SCALE, M, frames, T, hw)
    torch.cuda.synchronize()


def test_rows_are_frame_indices_batches_add_and_two_runs_are_the_same_bits():
    B, T, H, W, M, thr = 4, 3, 65, 63, 8, THRS[4]
    C = E.cols(M, len(thr))
    batches = [E.radar_stack(M, B * T, H, W, seed) for seed in (1, 2)]
    refs = [E.frame_rows(t, m, thr, SCALE).reshape(B, T, C) for t, m in batches]
    assert not (refs[0].sum(0) == refs[0].reshape(T, B, C).sum(1)).all(), "f mod T and f / T coincide on this data: nothing is tested"
    start = np.arange(T * C, dtype=np.float64).reshape(T, C) * 3.0      # the table is ADDED to
    tables = []
    for _ in range(2):
        table = _dev(start.ravel().copy())
        for i, (t, m) in enumerate(batches):
            _accum(_dev(m), B * T * H * W, T * H * W, H * W, _dev(t), table, thr, M, T, H * W)
            want = start + sum(r.sum(0) for r in refs[:i + 1])
            assert (table.view(T, C).cpu().numpy() == want).all(), f"after batch {i}"
        tables.append(table)
    assert torch.equal(tables[0].view(torch.int64), tables[1].view(torch.int64)), "the same calls on a fresh table give other bits"
    hold = torch.full((T * C + 8,), -7.0, dtype=torch.float64, device=DEV)
    hold[:T * C] = 0.0
    t, m = batches[0]
    _accum(_dev(m), B * T * H * W, T * H * W, H * W, _dev(t), hold, thr, M, T, H * W)
    assert bool((hold[T * C:] == -7.0).all()) and (hold[:T * C].view(T, C).cpu().numpy() == refs[0].sum(0)).all(), "a write behind the table"


@pytest.mark.parametrize("H,W", [(33, 32), (65, 63)], ids=["quads", "odd"])
def test_held_strides_slices_of_wider_tensors_and_bases_off_by_one_float(H, W):
    B, T, M, thr, hw = 2, 3, 4, THRS[4], H * W
    C = E.cols(M, len(thr))
    t, m = E.radar_stack(M, B * T, H, W, 3)
    tgt, mem = _dev(t), _dev(m)
    want = _table(T, M, len(thr))
    _accum(mem, B * T * hw, T * hw, hw, tgt, want, thr, M, T, hw)
    assert (want.view(T, C).cpu().numpy() == E.frame_rows(t, m, thr, SCALE).reshape(B, T, C).sum(0)).all()
    # a member stride of 0: M copies of member 1; through the op the broadcast view is read as it is
    got = _table(T, M, len(thr))
    _accum(mem[1], 0, T * hw, hw, tgt, got, thr, M, T, hw)
    ref = E.frame_rows(t, np.broadcast_to(m[1], m.shape), thr, SCALE)
    assert (got.view(T, C).cpu().numpy() == ref.reshape(B, T, C).sum(0)).all() and (ref[:, 4:6] == 0).all(), "a held member"
    assert (ops.ensemble_table(tgt, mem[1].expand(M, B * T, H, W), thr, SCALE).cpu().numpy() == ref).all()
    # a frame stride of 0: every member's first frame of a sample held over the T frame indices (the persistence shape)
    got = _table(T, M, len(thr))
    _accum(mem, B * T * hw, T * hw, 0, tgt, got, thr, M, T, hw)
    held = m.reshape(M, B, T, H, W)[:, :, :1].repeat(T, axis=2).reshape(M, B * T, H, W)
    assert (got.view(T, C).cpu().numpy() == E.frame_rows(t, held, thr, SCALE).reshape(B, T, C).sum(0)).all(), "a held frame"
    one = mem[:, :1].expand(M, B * T, H, W)
    assert (ops.ensemble_table(tgt, one, thr, SCALE).cpu().numpy() == E.frame_rows(t, np.broadcast_to(m[:, :1], m.shape), thr, SCALE)).all()
    # the members as frames 1..T of a (M, B, T + 2, H, W) tensor
    wide = torch.full((M, B, T + 2, H, W), 0.9, dtype=torch.float32, device=DEV)
    wide[:, :, 1:T + 1] = mem.view(M, B, T, H, W)
    got = _table(T, M, len(thr))
    _accum(wide[:, :, 1:], B * (T + 2) * hw, (T + 2) * hw, hw, tgt, got, thr, M, T, hw)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "a slice of a wider tensor"
    # both fields one float into a buffer: 4-byte aligned only
    hold_m, hold_t = torch.zeros(mem.numel() + 1, device=DEV), torch.zeros(tgt.numel() + 1, device=DEV)
    off_m, off_t = hold_m[1:].view(mem.shape), hold_t[1:].view(tgt.shape)
    off_m.copy_(mem), off_t.copy_(tgt)
    assert off_m.data_ptr() % 16 == 4 and off_t.data_ptr() % 16 == 4
    got = _table(T, M, len(thr))
    _accum(off_m, B * T * hw, T * hw, hw, off_t, got, thr, M, T, hw)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "bases one float off the 16-byte boundary"
    assert (ops.ensemble_table(off_t, off_m, thr, SCALE).cpu().numpy() == E.frame_rows(t, m, thr, SCALE)).all()


def test_the_control_and_the_exceedance_marginals_equal_the_point_wise_counts(monkeypatch):
    H, W, M = 40, 52, 8
    t, m = E.radar_stack(M, 3, H, W, 9)
    tgt, mem = _dev(t), _dev(m)
    thr = THRS[4]
    with guarded_workspaces(monkeypatch) as g:
        got = ops.ensemble_table(tgt, mem, thr, SCALE).cpu().numpy()
        twins = ops.ensemble_table(tgt, mem[:1].expand(2, 3, H, W), thr, SCALE).cpu().numpy()     # the control alone, twice
        g.check()
        assert g.calls == 0, "adnm_valid_ens_accum needs no workspace"
    cnt = ops.pool_counts(tgt, mem[0], thr, SCALE, ((1, 1),)).to(torch.int64).cpu().numpy()[:, 0].reshape(3, len(thr), 4)     # TP, FN, FP, TN
    at, at2 = 7 + (M + 1) ** 2, 7 + 9
    for k in range(len(thr)):
        x = got[:, at + 2 * k * (M + 1):at + 2 * (k + 1) * (M + 1)].reshape(3, 2, M + 1)
        assert (x[:, 1].sum(axis=1) == cnt[:, k, 0] + cnt[:, k, 1]).all() and (x[:, 0].sum(axis=1) + got[:, 1] == cnt[:, k, 2] + cnt[:, k, 3]).all(), "the target's events"
        x2 = twins[:, at2 + 6 * k:at2 + 6 * (k + 1)].reshape(3, 2, 3)
        assert (x2[:, :, 1] == 0).all() and (x2[:, 1, 2] == cnt[:, k, 0]).all() and (x2[:, 1, 0] == cnt[:, k, 1]).all() and (x2[:, 0, 2] == cnt[:, k, 2]).all()
        assert (x2[:, 0, 0] + twins[:, 1] == cnt[:, k, 3]).all(), "the control's events"
    # at a value scale of 1 the levels are 0 and 1, and |x_0 - y| is a miss or a false alarm
    one = ops.ensemble_table(tgt, mem, [1.0], 1.0).cpu().numpy()
    c1 = ops.pool_counts(tgt, mem[0], [1.0], 1.0, ((1, 1),)).to(torch.int64).cpu().numpy()[:, 0]
    assert (one[:, 2] == c1[:, 1] + c1[:, 2]).all() and int(one[:, 2].sum()) > 0, "S0"


# ------------------------------------------------------------------------------------------------ 3. the product
@pytest.mark.parametrize("M", list(range(2, 17)))
def test_the_product_equals_the_float32_loop_bit_for_bit_for_every_count(M):
    H, W = 6, 4 * (M + 1)
    rng = np.random.default_rng(M)
    mem = rng.uniform(0.0, 0.3, (M, 2, H, W)).astype(np.float32) * np.float32(1.0 / 3.0)
    col = np.arange(W) % (M + 1)
    for i in range(M):      # pixel column x has x mod (M + 1) members at or above 35: every count c = 0 .. M
        mem[i, :, :, col > i] += np.float32(0.5)
    thr = THRS[8]
    for K in (0, 1, 8):
        for off in (0, 1):      # aligned, and one float into a buffer
            hold = torch.zeros(mem.size + off, device=DEV)
            md = hold[off:].view(mem.shape)
            md.copy_(_dev(mem))
            assert md.data_ptr() % 16 == 4 * off
            mean, prob = ops.ensemble_product(md, thr[:K], SCALE if K else None)
            want_mean, want_prob = E.product(mem, thr[:K], SCALE)
            assert torch.equal(_bits(mean).cpu(), _bits(torch.from_numpy(want_mean))), (M, K, off, "mean")
            if K:
                assert prob.shape == (K, 2, H, W) and torch.equal(_bits(prob).cpu(), _bits(torch.from_numpy(want_prob))), (M, K, off, "prob")
            else:
                assert prob is None
    k35 = thr.index(35.0)
    assert sorted(set((want_prob[k35] * M).round().astype(int).ravel().tolist())) == list(range(M + 1)), "every count occurs"


def test_the_product_writes_every_element_and_takes_held_strides(monkeypatch):
    for shape in ((3, 2, 5, 7), (8, 3, 64, 65), (16, 1, 1, 4097), (4, 2, 32, 32)):
        _, m = E.radar_stack(shape[0], shape[1], shape[2], shape[3], 11)
        md = _dev(m)
        recs = []
        for pattern in (0, 1):
            with poisoned_outputs(monkeypatch, pattern) as p:
                mean, prob = ops.ensemble_product(md, THRS[4], SCALE)
                torch.cuda.synchronize()
                recs.append(p.records)
        assert len(recs[0]) == 2 and unwritten(*recs) == {}, shape
        want_mean, want_prob = E.product(m, THRS[4], SCALE)
        ok = ~np.isnan(want_mean)      # (a NaN member gives a NaN mean on both sides; its payload is not promised)
        assert (np.isnan(mean.cpu().numpy()) == ~ok).all() and (mean.cpu().numpy()[ok] == want_mean[ok]).all() and (prob.cpu().numpy() == want_prob).all(), shape
        held, _ = ops.ensemble_product(md[1].expand(shape), (), None)
        assert torch.equal(_bits(held).cpu(), _bits(torch.from_numpy(E.product(np.broadcast_to(m[1], shape), (), None)[0])))


# ------------------------------------------------------------------------------------------------ 4. the Validator through the captured graph
T_OUT = 4


class _Drift(torch.nn.Module):
    """a stand-in forecast that is NOT equivariant: the last input frame, moved one pixel more to the right and weakened with every lead
    (a flip reverses the drift).  roll and one fp32 multiply: exact on the CPU and on the device alike"""

    def forward(self, x):
        last = x[:, -1, 0].float()
        return torch.stack([torch.roll(last, t + 1, dims=-1) * (1.0 - 0.125 * t) for t in range(T_OUT)], dim=1)


class _Point(torch.nn.Module):
    """an equivariant stand-in: point-wise in space"""

    def forward(self, x):
        last = x[:, -1, 0].float()
        return torch.stack([last * (1.0 - 0.125 * t) for t in range(T_OUT)], dim=1)


def _cpu_members(module, x, codes):
    """the yardstick's members: g^-1(module(g(x))) with torch flips on the CPU -> (M, B, T, H, W)"""
    xc = x.cpu()
    return torch.stack([E.g_inv(module(E.g(xc, c)), c) for c in codes])


def _data(B, H, W, batches, seed):
    rng = np.random.default_rng(seed)
    base = 1.2 * E.blobs(rng, batches * B, H, W) + rng.normal(0.0, 0.004, size=(batches * B, H, W))
    base = np.where(base < np.quantile(base, 0.8), 0.0, base)
    samples = _dev(np.stack([np.roll(base, j, axis=2) for j in range(5 + T_OUT)], axis=1).astype(np.float32))
    return samples, [(samples[i:i + B, :5, None].contiguous(), samples[i:i + B, 5:, None].contiguous()) for i in range(0, batches * B, B)]


def _without(res, key="ensemble"):
    out = {k: v for k, v in res.items() if k != key}
    if "per_lead" in out:
        out["per_lead"] = {k: v for k, v in res["per_lead"].items() if k != key}
    return out


@pytest.mark.parametrize("codes", [True, (0, 1, 2, 7)], ids=["M8", "M4"])
def test_validator_members_and_table_equal_the_yardstick_beside_the_other_scores(codes):
    from adnm_hip.validate import Validator, ensemble_doubles, ensemble_entries
    from models.loss import RainfallLoss
    from test_tracks_host import _same_tree
    B, H, W, thr = 2, 32, 32, THRS[4]
    want_codes = tuple(range(8)) if codes is True else codes
    M, n = len(want_codes), len(thr)
    C = E.cols(M, n)
    _, data = _data(B, H, W, 2, 21)
    options = dict(fss=(1, 9), persistence=True, nprob=(3,), tracks=True)
    val = Validator(_Drift(), RainfallLoss(), T_OUT, SCALE, thr, ensemble=codes, **options)
    old = Validator(_Drift(), RainfallLoss(), T_OUT, SCALE, thr, **options)     # a stand-in that returns the control's forecast: the same module
    try:
        total = np.zeros((T_OUT, C), dtype=np.int64)
        for x, tgt in data:
            pred = val.step(x, tgt)
            ref = old.step(x, tgt)
            want = _cpu_members(_Drift(), x, want_codes)
            got = val.members(x)
            assert got.shape == (M, B, T_OUT, H, W) and torch.equal(_bits(got).cpu(), _bits(want)), "the members"
            assert pred.shape == ref.shape and torch.equal(_bits(pred), _bits(ref)) and pred.data_ptr() == got.data_ptr(), "a step returns the control"
            assert not torch.equal(got[1], got[0]), "the drifting stand-in is not equivariant"
            total += E.table(tgt[:, :, 0].cpu().numpy().reshape(B * T_OUT, H, W), want.numpy().reshape(M, B * T_OUT, H, W), thr, SCALE, T_OUT)
        parts = {p.name: p for p in val._parts}
        assert [p.name for p in val._parts][-2:] == ["ensemble", "tracks"] and val._block.numel() == old._block.numel() + ensemble_doubles(T_OUT, n, M)
        e = parts["ensemble"]
        tab = val._block[e.offset:e.offset + e.size].view(T_OUT, C)
        assert (tab.cpu().numpy() == total).all() and total[:, 4].min() > 0, "the table"
        # everything in front of the new table, and the tracks behind it, are the other Validator's bits
        assert torch.equal(val._block[:e.offset].view(torch.int64), old._block[:e.offset].view(torch.int64))
        assert torch.equal(val._block[e.offset + e.size:].view(torch.int64), old._block[e.offset:].view(torch.int64))
        res, plain = val.done(per_lead=True), old.done(per_lead=True)
        assert repr(_without(res)) == repr(plain), "an existing entry moved"
        assert list(res)[-3:] == ["ensemble", "tracks", "per_lead"] and list(res["per_lead"])[-1] == "ensemble"
        assert _same_tree(res["ensemble"], ensemble_entries(total.sum(axis=0), M, thr)) and _same_tree(res["per_lead"]["ensemble"], ensemble_entries(total, M, thr))
        assert res["ensemble"]["pixels"] == 2 * B * T_OUT * H * W and res["ensemble"]["crps"] > 0.0 and res["ensemble"]["spread"] > 0.0
        # a second epoch replays the graph: the same bits; and a step allocates nothing
        block = val._block.clone()
        val.done(reset=True)
        assert float(val._block.abs().sum()) == 0.0
        for x, tgt in data:
            val.step(x, tgt)
        assert torch.equal(val._block.view(torch.int64), block.view(torch.int64))
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        val.step(*data[0])
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    finally:
        val.close()
        old.close()


def test_validator_an_equivariant_model_has_no_spread_and_none_changes_nothing():
    from adnm_hip.validate import Validator
    from models.loss import RainfallLoss
    B, H, W, thr = 2, 32, 32, THRS[4]
    _, data = _data(B, H, W, 1, 22)
    x, tgt = data[0]
    val = Validator(_Point(), RainfallLoss(), T_OUT, SCALE, thr, ensemble=True)
    none = Validator(_Point(), RainfallLoss(), T_OUT, SCALE, thr, ensemble=None)
    plain = Validator(_Point(), RainfallLoss(), T_OUT, SCALE, thr)
    try:
        val.step(x, tgt), none.step(x, tgt), plain.step(x, tgt)
        mem = val.members(x)
        assert all(torch.equal(_bits(mem[m]), _bits(mem[0])) for m in range(8)), "every member equals the control"
        e = next(p for p in val._parts if p.name == "ensemble")
        tab = val._block[e.offset:e.offset + e.size].view(T_OUT, -1)
        assert float(tab[:, 4].abs().sum()) == 0.0 and float(tab[:, 5].abs().sum()) == 0.0 and float(tab[:, 2].sum()) > 0.0, "S2 = V = 0"
        res = val.done()
        assert res["ensemble"]["spread"] == 0.0 and res["ensemble"]["crps"] == res["ensemble"]["mae_control"]
        # ensemble=None: the keys, the block and the graph's entry are what they were
        assert none._block.numel() == plain._block.numel() and torch.equal(none._block.view(torch.int64), plain._block.view(torch.int64))
        assert repr(none.done()) == repr(plain.done()) and "ensemble" not in none.done()
        ent = next(iter(none._fwd._graphs.values()))
        assert ent["members"] is None and ent["xin"] is None and ent["codes"] is None
        with pytest.raises(RuntimeError, match="ensemble="):
            none.members(x)
        # one number of members for the Validator's lifetime
        val.done(reset=True)
        wide = torch.zeros(B, 5, 1, 32, 48, device=DEV), torch.zeros(B, T_OUT, 1, 32, 48, device=DEV)
        with pytest.raises(RuntimeError, match="one number of members"):
            val.step(*wide)
    finally:
        val.close(), none.close(), plain.close()


def test_validator_step_from_a_resident_dataset():
    from adnm_hip.dataio import ResidentDataset
    from adnm_hip.validate import Validator
    from models.loss import RainfallLoss
    B, H, W, thr = 2, 32, 32, THRS[4]
    samples, _ = _data(B, H, W, 3, 23)
    feed = ResidentDataset.from_frames(samples, 5, B, DEV, shuffle=False)
    twin = ResidentDataset.from_frames(samples, 5, B, DEV, shuffle=False)
    feed.begin_epoch(), twin.begin_epoch()
    va = Validator(_Drift(), RainfallLoss(), T_OUT, SCALE, thr, ensemble=(0, 1, 4))
    vb = Validator(_Drift(), RainfallLoss(), T_OUT, SCALE, thr, ensemble=(0, 1, 4))
    try:
        for i in range(3):      # the first batch captures, the later ones land in the graph's static buffers
            out = va.step_from(feed)
            x, tgt = twin.fetch()
            ref = vb.step(x, tgt)
            assert torch.equal(_bits(out), _bits(ref)) and torch.equal(_bits(va.members(x)).cpu(), _bits(_cpu_members(_Drift(), x, (0, 1, 4)))), i
        torch.cuda.synchronize()
        assert torch.equal(va._block.view(torch.int64), vb._block.view(torch.int64)) and va.done()["ensemble"]["members"] == 3
    finally:
        va.close(), vb.close()


def test_the_real_model_once_members_equal_a_plain_forward_of_the_transformed_batch():
    """the same kernels at the same shapes (batch 8), so bit equality is what the suite's replay-determinism tests predict"""
    from adnm_hip import recipe
    from adnm_hip.evaluator import GraphedForward
    from adnm_hip.validate import Validator
    from models.ADNMUNet import create_ADNMUNet
    from models.loss import enRainfallLoss
    ops.set_mfma_precision("f32")
    model = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(model)
    model = model.to(DEV).eval()
    frames = recipe.radar_batch(1, 25, 64, name="ensemble.e2e").to(DEV)
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    codes = tuple(range(8))
    val = Validator(model, enRainfallLoss(0.57, 0.25, gamma=0.0), 20, SCALE, ensemble=True)
    fwd = GraphedForward(model)
    try:
        val.step(x, tgt)
        got = val.members(x)
        batch = torch.cat([E.g(x, c) for c in codes])      # the torch-made g-batch, member-major
        out = fwd(batch)
        want = torch.stack([E.g_inv(out[m:m + 1, :, 0], c) for m, c in enumerate(codes)])
        assert got.shape == want.shape == (8, 1, 20, 64, 64)
        assert torch.equal(_bits(got), _bits(want)), f"relative L2 {float((got - want).norm() / want.norm()):.3e}"
        assert not torch.equal(got[1], got[0]), "the network is not exactly equivariant: the members differ"
        res = val.done()
        assert res["ensemble"]["members"] == 8 and res["ensemble"]["pixels"] == 20 * 64 * 64 and res["ensemble"]["spread"] > 0.0
    finally:
        val.close()
        fwd.close()


# ------------------------------------------------------------------------------------------------ 5. the Forecaster
def _palette():
    from adnm_hip.forecast import Palette
    return Palette([0.0, 20.0, 35.0, 50.0, 255.0], np.array([[0, 0, 0, 255], [0, 200, 0, 255], [255, 200, 0, 255], [255, 0, 0, 255]], dtype=np.uint8))


@pytest.mark.parametrize("raw", [False, True], ids=["fp32", "uint8"])
def test_forecaster_members_mean_and_probability_equal_the_yardstick(raw):
    from adnm_hip.forecast import Forecaster
    B, S, thr = 2, 32, [20.0, 35.0]
    samples, data = _data(B, S, S, 1, 24)
    if raw:
        x = (samples[:B, :5].clamp(0, 1) * 255.0).to(torch.uint8).contiguous()      # (B, T_in, H0, W0) bytes at the model's size: the resize is the identity
    else:
        x = data[0][0]
    codes = (0, 3, 5, 6)
    fc = Forecaster(_Drift(), _palette(), pixel_scale=SCALE, size=S, ensemble=dict(members=codes, thresholds=thr))
    plain = Forecaster(_Drift(), _palette(), pixel_scale=SCALE, size=S)      # a stand-in that returns the control's forecast: the same module
    none = Forecaster(_Drift(), _palette(), pixel_scale=SCALE, size=S, ensemble=None)
    try:
        res, ref, off = fc(x), plain(x), none(x)
        xin = next(iter(plain._fwd._graphs.values()))["xin"] if raw else x      # what the model sees: the ingested frames
        want = _cpu_members(_Drift(), xin, codes)
        assert res.members.shape == (4, B, T_OUT, S, S) and torch.equal(_bits(res.members).cpu(), _bits(want)), "members"
        mean, prob = E.product(want.numpy(), thr, SCALE)
        assert res.ens_mean.shape == (B, T_OUT, S, S) and torch.equal(_bits(res.ens_mean).cpu(), _bits(torch.from_numpy(mean))), "mean"
        assert res.ens_prob.shape == (2, B, T_OUT, S, S) and torch.equal(_bits(res.ens_prob).cpu(), _bits(torch.from_numpy(prob))), "prob"
        assert 0.0 < float(res.ens_prob.mean()) < 1.0 and len(torch.unique(res.ens_prob)) > 2
        assert torch.equal(_bits(res.pred), _bits(ref.pred)) and torch.equal(res.fields, ref.fields) and torch.equal(res.strip, ref.strip) and res.prob is None
        coloured = fc.render(res.ens_mean)
        assert coloured.fields.shape == res.fields.shape and coloured.strip.shape == res.strip.shape
        # ensemble=None: nothing new in the graph's entry or the result
        assert off.members is None and off.ens_mean is None and off.ens_prob is None and torch.equal(off.fields, ref.fields)
        ent = next(iter(none._fwd._graphs.values()))
        assert ent["xmem"] is None and ent["codes"] is None and ent["members"] is None and ent["ens_mean"] is None
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        fc(x)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    finally:
        fc.close(), plain.close(), none.close()
