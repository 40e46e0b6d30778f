"""Radially averaged power spectra on the GPU (csrc/spectrum.hip: adnm_valid_spectrum_accum; ops.power_spectrum; Validator(spectrum=)):
against numpy.fft in float64 on the CPU (spectrum_ref), with a bar per case of 4 times what a float32 transform on the CPU (scipy's,
complex64) deviates from float64 on the same fields; known answers; bit-reproducibility; accumulation; addressing; the workspace contract;
and end to end through the captured graph.

Figures of the hardware run, per case, in profiles/spectrum_error.txt: the GPU's largest per-bin deviation lies between 0.5 and 1.35
times the CPU float32 transform's own (1.4e-7 at 8 x 8 up to 1.0e-4 at 512 x 8 with sigma 2), against the bar of 4 times."""
import numpy as np
import pytest
import torch

import spectrum_ref as S
from adnm_hip import lib, ops, recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = S.SCALE

_fields, _refs = {}, {}


def _pair(case):
    """the CPU fields of a case, made once and never written to"""
    if case not in _fields:
        _fields[case] = S.fields(*case)
    return _fields[case]


def _ref(case):
    """(float64 sums, the corners' sums, the float32 restatement's two deviation figures) of a case, made once"""
    if case not in _refs:
        t, p = _pair(case)
        sums, corners = S.ref_sums(t, p, SCALE, corners=True)
        _refs[case] = (sums, corners, S.deviation(S.ref_sums_f32(t, p, SCALE), sums))
        sums.setflags(write=False)
    return _refs[case]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _table(T, H, W):
    return torch.zeros(lib.query("adnm_valid_spectrum_block_bytes", T, H, W) // 8, dtype=torch.float64, device=DEV)


def _accum(pred_ptr, sample_stride, frame_stride, tgt, table, T, ws=None):
    """tgt: (frames, H, W) on the device, contiguous or a slice that is; the forecast by address and strides"""
    frames, H, W = tgt.shape
    nb = lib.query("adnm_valid_spectrum_accum_ws_bytes", frames, T, H, W)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV) if ws is None else ws
    lib.call("adnm_valid_spectrum_accum", pred_ptr, sample_stride, frame_stride, tgt.data_ptr(), table.data_ptr(), SCALE, ws.data_ptr(), nb, frames, T, H, W,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return nb


# ------------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_power_spectrum_against_numpy_fft_in_float64(case):
    """(8, 8): one butterfly pattern per axis; (16, 64) / (64, 16): H != W, the L/H scaling, row groups against columns; (32, 32) x 3:
    the fold; (128, 128): the workload's size, white and with a spectrum of eight decades; (512, 8) / (8, 512): the longest against the
    shortest, along either axis.
    The bar: 4 x the deviation of the CPU's own float32 transform from float64 on the same fields, per bin, relative to the bin (C:
    relative to sqrt(P_o P_f)); and no bin off by more than 1e-6 of the frame's total power; and Parseval with the yardstick's corners."""
    t, p = _pair(case)
    ref, corners, (cpu_rel, cpu_tot) = _ref(case)
    got = ops.power_spectrum(_dev(t), _dev(p), SCALE)
    assert got.dtype == torch.float64 and tuple(got.shape) == ref.shape == (case[0], max(case[1:3]) // 2, 3)
    got = got.cpu().numpy()
    rel, tot = S.deviation(got, ref)
    o, f = S.clipped(t, SCALE), S.clipped(p, SCALE)
    want = np.stack([(o * o).sum(axis=(1, 2)), (f * f).sum(axis=(1, 2)), (o * f).sum(axis=(1, 2))], axis=1)
    pars = float((np.abs(got.sum(axis=1) + corners - want) / np.stack([want[:, 0], want[:, 1], np.sqrt(want[:, 0] * want[:, 1])], axis=1)).max())
    print(f"spectrum {S.case_id(case)}: per-bin relative deviation from float64: CPU float32 {cpu_rel:.3e}, GPU {rel:.3e} (bar {4 * cpu_rel:.3e}); "
          f"relative to the frame's power: CPU {cpu_tot:.3e}, GPU {tot:.3e} (bar 1e-6); Parseval GPU {pars:.3e}")
    assert rel <= 4 * cpu_rel, f"a bin is off by {rel:.3e} of itself, the CPU's float32 transform by {cpu_rel:.3e}"
    assert tot <= 1e-6, f"a bin is off by {tot:.3e} of the frame's total power"
    assert pars <= 4 * cpu_rel, f"Parseval: the sums and the corners miss the field's energy by {pars:.3e}"


# ------------------------------------------------------------------------------------------------ 2. known answers
def test_a_constant_frame_has_its_power_in_bin_zero():
    v = np.full((2, 16, 64), 0.5, dtype=np.float32)
    v[1] = 0.25
    got = ops.power_spectrum(_dev(v), _dev(v[::-1]), SCALE).cpu().numpy()
    for i, (a, b) in enumerate(((0.5, 0.25), (0.25, 0.5))):
        a, b = float(np.float32(a) * np.float32(SCALE)), float(np.float32(b) * np.float32(SCALE))
        want = np.array([16 * 64 * a * a, 16 * 64 * b * b, 16 * 64 * a * b])
        assert (np.abs(got[i, 0] - want) <= 1e-6 * want).all(), (i, got[i, 0], want)
        assert (np.abs(got[i, 1:]) <= 1e-6 * want).all(), (i, np.abs(got[i, 1:]).max(axis=0), want)


def test_a_cosine_lands_in_the_bin_the_integer_rule_gives():
    """(16, 64), L/H = 4: (a, b) = (2, 3) is wavenumber (8, 3), bin 9; (3, 2) is (12, 2), bin 12; without the L/H factor both would be
    sqrt(13), bin 4"""
    H, W, amp = 16, 64, 0.4
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    waves = [(2, 3, 9), (3, 2, 12)]
    v = np.stack([0.5 + amp * np.cos(2 * np.pi * (a * y / H + b * x / W)) for a, b, _ in waves]).astype(np.float32)
    assert S.bin_image(H, W)[2, 3] == 9 and S.bin_image(H, W)[3, 2] == 12
    got = ops.power_spectrum(_dev(v), _dev(v), SCALE).cpu().numpy()
    power = (amp * SCALE) ** 2 * H * W / 2          # two coefficients of (amp * scale * H W / 2)^2 / (H W) each
    for i, (a, b, r) in enumerate(waves):
        assert abs(got[i, r, 0] - power) <= 1e-5 * power, (a, b, got[i, r, 0], power)
        rest = np.delete(got[i, :, 0], [0, r])
        assert (rest <= 1e-6 * power).all(), (a, b, int(np.argmax(rest)), rest.max(), power)


def test_equal_fields_give_equal_columns_and_a_zero_forecast_gives_zeros_bit_for_bit():
    for case in (S.CASES[1], S.CASES[4]):
        t = _dev(_pair(case)[0])
        same = ops.power_spectrum(t, t.clone(), SCALE)
        assert float(same[..., 0].min()) > 0
        assert torch.equal(_bits(same[..., 0]), _bits(same[..., 1])) and torch.equal(_bits(same[..., 0]), _bits(same[..., 2]))
        none = ops.power_spectrum(t, torch.zeros_like(t), SCALE)
        assert torch.equal(_bits(none[..., 0]), _bits(same[..., 0])) and float(none[..., 1:].abs().max()) == 0.0
        low = ops.power_spectrum(t, torch.full_like(t, -3.0), SCALE)       # clipped to 0
        assert float(low[..., 1:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 3. determinism and accumulation
def test_rows_are_frame_indices_batches_add_and_the_bits_repeat():
    B, T, H, W = 2, 2, 32, 32
    batches = [S.fields(B * T, H, W, 0, seed) for seed in (11, 12)]
    one = [ops.power_spectrum(_dev(t), _dev(p), SCALE).cpu().numpy().reshape(B, T, H // 2, 3) for t, p in batches]      # one-shot, per frame
    assert not np.allclose(one[0].sum(0), one[0].reshape(T, B, H // 2, 3).sum(1), rtol=1e-3), "f mod T and f / T coincide on this data: nothing is tested"
    tables = []
    for _ in range(2):
        table = _table(T, H, W)
        for i, (t, p) in enumerate(batches):
            pd = _dev(p)
            _accum(pd.data_ptr(), T * H * W, H * W, _dev(t), table, T)
            if not tables:
                want = np.zeros((T, H // 2, 3))
                for s in one[:i + 1]:                  # the device's order: a batch's samples ascending, then the table += the batch
                    want = want + (s[0] + s[1])
                got = table.view(T, H // 2, 3).cpu().numpy()
                assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), f"after batch {i}"
        tables.append(table)
    assert torch.equal(_bits(tables[0]), _bits(tables[1])), "the same calls on a fresh table give other bits"


# ------------------------------------------------------------------------------------------------ 4. addressing
def test_frame_stride_zero_is_the_expanded_copy():
    B, T, T_in, H, W = 2, 3, 2, 16, 64
    t = _dev(S.fields(B * T, H, W, 2, 21)[0])
    x = _dev(S.fields(B * T_in, H, W, 2, 22)[1]).view(B, T_in, H, W)
    a, b = _table(T, H, W), _table(T, H, W)
    _accum(x.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, t, a, T)          # the last input frame, held over the horizon
    held = x[:, -1:].expand(B, T, H, W).contiguous().view(B * T, H, W)
    _accum(held.data_ptr(), T * H * W, H * W, t, b, T)
    assert torch.equal(_bits(a), _bits(b))
    want = S.ref_sums(t.cpu().numpy(), held.cpu().numpy(), SCALE).reshape(B, T, W // 2, 3).sum(0)
    cpu_rel = S.deviation(S.ref_sums_f32(t.cpu().numpy(), held.cpu().numpy(), SCALE).reshape(B, T, W // 2, 3).sum(0), want)[0]
    assert S.deviation(a.view(T, W // 2, 3).cpu().numpy(), want)[0] <= 4 * cpu_rel


@pytest.mark.parametrize("H,W", [(64, 16), (128, 128)])
def test_bases_one_float_off_the_16_byte_boundary_and_a_slice_of_a_wider_tensor(H, W):
    B, T = 2, 2
    tn, pn = S.fields(B * T, H, W, 2, 31)
    tgt, pred = _dev(tn), _dev(pn)
    want = _table(T, H, W)
    _accum(pred.data_ptr(), T * H * W, H * W, tgt, want, T)
    hold_p, hold_t = (torch.zeros(B * T * H * W + 1, dtype=torch.float32, device=DEV) for _ in range(2))
    off_p, off_t = hold_p[1:].view(B * T, H, W), hold_t[1:].view(B * T, H, W)
    off_p.copy_(pred), off_t.copy_(tgt)
    assert off_p.data_ptr() % 16 == 4 and off_t.data_ptr() % 16 == 4 and pred.data_ptr() % 16 == 0 and tgt.data_ptr() % 16 == 0
    got = _table(T, H, W)
    _accum(off_p.data_ptr(), T * H * W, H * W, off_t, got, T)
    assert torch.equal(_bits(got), _bits(want)), "float-by-float loads give other bits than 16-byte loads"
    wide = torch.full((B, T + 2, H, W), 0.9, dtype=torch.float32, device=DEV)
    wide[:, 1:T + 1] = pred.view(B, T, H, W)
    got = _table(T, H, W)
    _accum(wide[:, 1:].data_ptr(), (T + 2) * H * W, H * W, tgt, got, T)
    assert torch.equal(_bits(got), _bits(want)), "a slice of a wider tensor"


# ------------------------------------------------------------------------------------------------ 5. the workspace contract
def test_the_call_stays_inside_its_workspace_and_does_not_read_what_it_held(monkeypatch):
    from util import guarded_workspaces
    for case in (S.CASES[1], S.CASES[6]):
        t, p = (_dev(a) for a in _pair(case))
        want = ops.power_spectrum(t, p, SCALE)
        with guarded_workspaces(monkeypatch) as g:
            got = ops.power_spectrum(t, p, SCALE)
            g.check()
            assert g.calls == 1 and g.records[0][2] == lib.query("adnm_valid_spectrum_accum_ws_bytes", case[0], case[0], case[1], case[2])
        assert torch.equal(_bits(got), _bits(want)), "the result depends on what the workspace held"


def test_nothing_behind_the_workspace_or_the_table_is_written():
    B, T, H, W = 2, 3, 64, 16
    tn, pn = S.fields(B * T, H, W, 2, 41)
    tgt, pred = _dev(tn), _dev(pn)
    nb = lib.query("adnm_valid_spectrum_accum_ws_bytes", B * T, T, H, W)
    cells, guard = T * (H // 2) * 3, 4096
    results = []
    for fill in (0x00, 0xFF):
        ws = torch.full((nb + guard,), fill, dtype=torch.uint8, device=DEV)
        ws[nb:] = 0xA5
        hold = torch.full((cells + 64,), -7.0, dtype=torch.float64, device=DEV)
        hold[:cells] = 0.0
        assert _accum(pred.data_ptr(), T * H * W, H * W, tgt, hold, T, ws=ws) == nb
        assert bool((ws[nb:] == 0xA5).all()), "a write behind ws_bytes"
        assert bool((hold[cells:] == -7.0).all()), "a write behind the table"
        results.append(hold[:cells].clone())
    assert torch.equal(_bits(results[0]), _bits(results[1])), "the result depends on what the workspace held"
    assert float(results[0].min()) != 0.0 and bool(torch.isfinite(results[0]).all())


# ------------------------------------------------------------------------------------------------ 6. non-finite input
def test_a_nan_pixel_spoils_its_own_row_only():
    T, H, W = 3, 32, 32
    tn, pn = (a.copy() for a in _pair(S.CASES[3]))
    clean, dirty = _table(T, H, W), _table(T, H, W)
    pd = _dev(pn)
    _accum(pd.data_ptr(), T * H * W, H * W, _dev(tn), clean, T)
    tn[1, 5, 7] = np.nan
    _accum(pd.data_ptr(), T * H * W, H * W, _dev(tn), dirty, T)          # the launch succeeds
    clean, dirty = clean.view(T, H // 2, 3), dirty.view(T, H // 2, 3)
    assert bool(torch.isnan(dirty[1, :, 0]).all()) and bool(torch.isnan(dirty[1, :, 2]).all()), "the NaN's frame: P_o and C of every bin"
    assert torch.equal(_bits(dirty[1, :, 1]), _bits(clean[1, :, 1])), "the forecast of that frame has no NaN"
    assert torch.equal(_bits(dirty[0]), _bits(clean[0])) and torch.equal(_bits(dirty[2]), _bits(clean[2])) and bool(torch.isfinite(clean).all())


# ------------------------------------------------------------------------------------------------ 7. the Validator end to end
def _model():
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(m)
    return m.to(DEV).eval()


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):       # inf - inf where both are inf: equal
        return a.shape == b.shape and bool(((np.isnan(a) & np.isnan(b)) | (a == b) | (np.abs(a - b) <= 1e-12 * np.abs(b))).all())


def test_validator_with_spectrum_end_to_end():
    from adnm_hip.validate import Validator, aggregate, block_doubles, spectrum_doubles
    from models.loss import enRainfallLoss
    model, crit, scale, T, thr = _model(), enRainfallLoss(0.57, 0.25, gamma=0.0), 255.0, 20, [20, 30, 35, 40]
    rng = np.random.default_rng(3)
    frames = np.stack([S.fields(25, 64, 64, 3, 50 + i)[0] for i in range(4)]).clip(0, 1) * 0.45 + rng.normal(0, 0.004, (4, 25, 64, 64))
    samples = _dev(frames.astype(np.float32))
    data = [(samples[i:i + 2, :5, None].contiguous(), samples[i:i + 2, 5:, None].contiguous()) for i in (0, 2)]
    val = Validator(model, crit, T, scale, thr, spectrum=True)
    plain = Validator(model, crit, T, scale, thr)
    full = Validator(model, crit, T, scale, thr, spectrum=True, fss=(1, 5), pools=(4,), persistence=True, advection=True)
    try:
        n0, R = block_doubles(T, len(thr))[0], 32
        assert spectrum_doubles(T, (64, 64)) == T * R * 3
        table = np.zeros((T, R, 3))
        for x, tgt in data:            # two steps through the captured graph
            val.step(x, tgt)
            ent = val._fwd.entry(x)
            one = ops.power_spectrum(ent["tgt"].view(2 * T, 64, 64), ent["pred"].view(2 * T, 64, 64), scale).cpu().numpy().reshape(2, T, R, 3)
            table = table + (one[0] + one[1])
            plain.step(x, tgt)
            full.step(x, tgt)
        assert val._block.numel() == plain._block.numel() + T * R * 3 and all(e.get("ws_spectrum") is None for e in plain._fwd._graphs.values())
        block = val._block.cpu().numpy()
        assert _close(block[n0:].reshape(T, R, 3), table) and (table[..., :2] > 0).all(), "the table at the end of the one allocation"
        res, old, both = val.done(per_lead=True), plain.done(per_lead=True), full.done(per_lead=True)
        want = aggregate(np.concatenate([block[:n0], table.ravel()]), thr, T, 64 * 64, 54 * 54, per_lead=True, spectrum=(64, 64))
        keys = ["wavenumber", "wavelength_px", "target", "forecast", "ratio", "coherence", "effective_resolution_px"]
        for got, exp in ((res["spectrum"], want["spectrum"]), (res["per_lead"]["spectrum"], want["per_lead"]["spectrum"])):
            assert list(got) == keys
            for k in keys:
                assert _close(got[k], exp[k]), k
        assert res["spectrum"]["target"].shape == (R,) and res["per_lead"]["spectrum"]["ratio"].shape == (T, R)
        assert res["per_lead"]["spectrum"]["effective_resolution_px"].shape == (T,) and (res["samples"], res["batches"]) == (4, 2)
        assert (np.abs(res["spectrum"]["coherence"][np.isfinite(res["spectrum"]["coherence"])]) <= 1 + 1e-6).all()
        print("spectrum end to end: ratio at bins 1, 8, 31:", res["spectrum"]["ratio"][[1, 8, 31]], "effective resolution", res["spectrum"]["effective_resolution_px"])
        # no existing behaviour moved: every key of the plain Validator, value for value, on the same batches
        assert set(res) == set(old) | {"spectrum"} and set(res["per_lead"]) == set(old["per_lead"]) | {"spectrum"}
        assert repr({k: res[k] for k in old if k != "per_lead"}) == repr({k: old[k] for k in old if k != "per_lead"})
        assert repr({k: res["per_lead"][k] for k in old["per_lead"]}) == repr(old["per_lead"])
        # the table really is last: with every other table in front of it, the same spectrum bit for bit
        assert set(both) == set(res) | {"pooled", "persistence", "fss", "fss_useful", "advection"}
        assert repr(both["spectrum"]) == repr(res["spectrum"]) and repr(both["per_lead"]["spectrum"]) == repr(res["per_lead"]["spectrum"])
        assert (full._block[-T * R * 3:].cpu().numpy().view(np.int64) == block[n0:].view(np.int64)).all()
        former = Validator(model, crit, T, scale, thr, fss=(1, 5), pools=(4,), persistence=True, advection=True)
        try:
            for x, tgt in data:
                former.step(x, tgt)
            was = former.done(per_lead=True)
            assert repr({k: both[k] for k in was if k != "per_lead"}) == repr({k: was[k] for k in was if k != "per_lead"})
            assert repr({k: both["per_lead"][k] for k in was["per_lead"]}) == repr(was["per_lead"])
        finally:
            former.close()
        # once the graph exists a step allocates nothing
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        val.step(*data[0])
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    finally:
        val.close()
        plain.close()
        full.close()


def test_a_frame_size_outside_the_limits_raises_from_the_first_step():
    from adnm_hip.validate import Validator
    from models.loss import RainfallLoss

    class LastFrames(torch.nn.Module):
        def forward(self, x):
            return x[:, -20:, 0].float() * 0.9

    x = torch.zeros(2, 25, 1, 96, 96, device=DEV)
    val = Validator(LastFrames(), RainfallLoss(), 20, SCALE, spectrum=True)
    plain = Validator(LastFrames(), RainfallLoss(), 20, SCALE)
    try:
        with pytest.raises(RuntimeError, match="adnm_valid_spectrum_accum's limits"):
            val.step(x, x[:, 5:].contiguous())
        plain.step(x, x[:, 5:].contiguous())          # without spectrum the frame size is no limit
        assert plain.done()["samples"] == 2
    finally:
        val.close()
        plain.close()
