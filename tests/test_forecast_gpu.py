"""Forecast fields and colour strips on the device (csrc/dataio.hip: adnm_forecast_render, ops.forecast_render,
adnm_hip.forecast.Forecaster) on the GPU.  Every comparison is exact byte equality: against matplotlib's own output
(tests/golden/forecast_render_*.npz) and against the numpy restatement that tests/test_forecast_host.py pins to it
(tests/forecast_ref.py), at the shapes where the indexing can go wrong, then end to end behind the captured forward."""
import numpy as np
import pytest
import torch

import forecast_ref as R
from adnm_hip import ops, recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"

_pal = {}


def _palette(name):
    if name not in _pal:
        _pal[name] = R.load_palette(name)
    return _pal[name]


def _np(t):
    return None if t is None else t.cpu().numpy()


def _check(pred, edges, rgba, scale, start, step, gap, fields=True, strip=True, what=""):
    """ops.forecast_render on `pred` (a numpy array) against the restatement, byte for byte"""
    f, s = ops.forecast_render(torch.from_numpy(pred).to(DEV), edges, rgba, scale, frame_start=start, frame_step=step, gap=gap, fields=fields, strip=strip)
    wf, ws = R.render(pred, edges, rgba, scale, start, step, gap)
    assert (f is None) == (not fields) and (s is None) == (not strip)
    if fields:
        assert f.dtype == torch.uint8 and tuple(f.shape) == wf.shape
        assert np.array_equal(_np(f), wf), f"{what}: {int((_np(f) != wf).sum())} of {wf.size} field bytes differ"
    if strip:
        assert s.dtype == torch.uint8 and tuple(s.shape) == ws.shape, (what, tuple(s.shape), ws.shape)
        assert np.array_equal(_np(s), ws), f"{what}: {int((_np(s) != ws).any(-1).sum())} of {ws.size // 4} strip pixels differ"
    return f, s


def _values(shape, seed, edges, scale):
    """uniform [0, 1) with values ON the edges and one float either side of them planted at every 7th pixel"""
    rng = np.random.default_rng(seed)
    p = rng.random(shape, dtype=np.float32)
    e = np.asarray(edges, dtype=np.float64) / (scale if scale else 1.0)
    near = np.concatenate([np.nextafter(e.astype(np.float32), np.float32(-np.inf)), e.astype(np.float32), np.nextafter(e.astype(np.float32), np.float32(np.inf))])
    near = near[(near >= 0) & (near * np.float32(scale if scale else 1.0) < 256)]
    flat = p.reshape(-1)
    flat[::7] = near[rng.integers(0, near.size, size=flat[::7].shape)]
    return p


# ------------------------------------------------------------------------------------------------ 1. matplotlib's own output
@pytest.mark.parametrize("name", ["shanghai", "laps"])
def test_op_vs_reference_fixture(name):
    z = R.load_fixture(name)
    edges, rgba = _palette(name)
    call = (1, 2, 10) if name == "shanghai" else (0, 1, 10)
    assert (int(z["frame_start"]), int(z["frame_step"]), int(z["gap"])) == call
    for pred in (torch.from_numpy(z["pred"]).to(DEV), torch.from_numpy(z["pred"]).to(DEV).unsqueeze(2)):   # (B, T, H, W) and (B, T, 1, H, W)
        f, s = ops.forecast_render(pred, edges, rgba, float(z["pixel_scale"]), frame_start=call[0], frame_step=call[1], gap=call[2])
        assert np.array_equal(_np(f), z["fields"]), f"{int((_np(f) != z['fields']).sum())} field bytes differ from the reference's"
        assert tuple(s.shape) == z["strip"].shape
        assert np.array_equal(_np(s), z["strip"]), f"{int((_np(s) != z['strip']).any(-1).sum())} strip pixels differ from the reference's PNG"


# ------------------------------------------------------------------------------------------------ 2. where the indexing can go wrong
SHAPES = [(1, 1, 1, 1),
          (2, 3, 5, 7),        # scalar path, odd everything
          (1, 4, 8, 8),        # vector path, one lane-group per row pair
          (3, 5, 16, 12),      # with gap 0 / 1 / 10: strip origins 16-, 4- and 8-byte aligned
          (1, 2, 4, 516)]      # a row longer than one workgroup's span
OUTPUTS = {"fields": (True, False), "strip": (False, True), "both": (True, True)}


@pytest.mark.parametrize("outputs", list(OUTPUTS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_vs_restatement(shape, outputs):
    fields, strip = OUTPUTS[outputs]
    T = shape[1]
    n = 0
    for form, scale in (("shanghai", 90.0), ("laps", 0.0)):
        edges, rgba = _palette(form)
        pred = _values(shape, sum(shape), edges, scale)
        for gap in (0, 1, 10):
            for start, step in ((0, 1), (1, 2), (4, 3)):
                if start >= T:
                    continue
                _check(pred, edges, rgba, scale, start, step, gap, fields, strip, what=f"{form} {shape} gap {gap} frames {start}::{step}")
                n += 1
    assert n >= 6


def test_frame_selection_outside_the_sequence_is_refused():
    edges, rgba = _palette("shanghai")
    pred = torch.zeros((1, 4, 8, 8), device=DEV)
    for start, step in ((4, 3), (0, 0), (-1, 1)):
        with pytest.raises(RuntimeError):
            ops.forecast_render(pred, edges, rgba, 90.0, frame_start=start, frame_step=step)


def test_fields_only_call_is_not_held_to_the_strip_limits():
    """2^20 frames of 1 x 16: the strip would be 2^24 pixels wide and is refused, the fields alone are not"""
    edges, rgba = _palette("shanghai")
    pred = torch.zeros((1, 1 << 20, 1, 16), device=DEV)
    pred[0, ::4099, 0, 5] = 0.5
    with pytest.raises(RuntimeError, match="pixels wide"):
        ops.forecast_render(pred, edges, rgba, 90.0, gap=0, fields=False, strip=True)
    f, s = ops.forecast_render(pred, edges, rgba, 90.0, gap=0, fields=True, strip=False)
    assert s is None and torch.equal(f, (pred * 90.0).to(torch.uint8)) and int(f.sum()) == 45 * len(range(0, 1 << 20, 4099))


# ------------------------------------------------------------------------------------------------ 3. all 256 bytes
def test_every_byte_value():
    edges = [8.0 * k for k in range(33)]                                           # 32 bins of 8 byte values
    rgba = np.array([[k, 255 - k, (37 * k) % 256, 255 - (k % 2)] for k in range(32)], dtype=np.uint8)
    k = np.arange(256, dtype=np.float64) / 255.0
    c = k.astype(np.float32)
    vals = np.concatenate([np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))])
    vals = vals[(vals >= 0) & (vals * np.float32(255.0) < 256)]
    pred = np.zeros((1, 2, 28, 28), dtype=np.float32)
    assert 760 <= vals.size <= 784
    pred[0, 0].reshape(-1)[:vals.size] = vals
    pred[0, 1].reshape(-1)[-vals.size:] = vals[::-1]
    f, _ = _check(pred, edges, rgba, 255.0, 0, 1, 3, what="all bytes")
    assert set(np.unique(_np(f)).tolist()) == set(range(256)), "not every byte value was produced"


# ------------------------------------------------------------------------------------------------ 4. outside the range
BAD = np.array([-1.0, -1e-30, 3.0, 255.5 / 90.0, 1e30, np.inf, -np.inf, np.nan], dtype=np.float32)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 4, 8, 12)], ids=lambda s: "x".join(map(str, s)))
def test_out_of_range_values_take_the_documented_clamp(shape):
    edges, rgba = _palette("shanghai")
    good = _values(shape, 5, edges, 90.0)
    bad = good.copy()
    pos = np.arange(3, good.size, 5)
    bad.reshape(-1)[pos] = BAD[np.arange(pos.size) % BAD.size]
    f, s = _check(bad, edges, rgba, 90.0, 0, 1, 10, what="byte form, out of range")
    fb = _np(f).reshape(-1)[pos]
    want = np.array([0, 0, 255, 255, 255, 255, 0, 0], dtype=np.uint8)[np.arange(pos.size) % BAD.size]
    assert np.array_equal(fb, want), "the clamp is: negative, -Inf, NaN -> 0; above 255, +Inf -> 255"
    # no dependence on the neighbours: everywhere else the bytes are those of the in-range tensor
    gf, gs = ops.forecast_render(torch.from_numpy(good).to(DEV), edges, rgba, 90.0, gap=10)
    keep = np.ones(good.size, dtype=bool)
    keep[pos] = False
    assert np.array_equal(_np(f).reshape(-1)[keep], _np(gf).reshape(-1)[keep])
    B, T, H, W = shape
    frames = lambda st: np.stack([_np(st)[:, :, j * (W + 10):j * (W + 10) + W] for j in range(T)], axis=1).reshape(-1, 4)   # (B, T, H, W) pixels of a strip
    assert np.array_equal(frames(s)[keep], frames(gs)[keep])
    # the float form: Inf bins like any value, NaN renders 0,0,0,0
    edges, rgba = _palette("laps")
    good = _values(shape, 6, edges, 0.0)
    bad = good.copy()
    bad.reshape(-1)[pos] = BAD[np.arange(pos.size) % BAD.size]
    f, s = _check(bad, edges, rgba, 0.0, 0, 1, 10, what="float form, out of range")
    nan = np.isnan(bad.reshape(-1))
    assert nan.sum() >= 2 and (frames(s)[nan] == 0).all() and (_np(f).reshape(-1)[nan] == 0).all()
    assert (frames(s)[bad.reshape(-1) == np.inf] == rgba[-1]).all() and (frames(s)[bad.reshape(-1) == -np.inf] == rgba[0]).all()
    gf, gs = ops.forecast_render(torch.from_numpy(good).to(DEV), edges, rgba, 0.0, gap=10)
    assert np.array_equal(_np(f).reshape(-1)[keep], _np(gf).reshape(-1)[keep]) and np.array_equal(frames(s)[keep], frames(gs)[keep])


# ------------------------------------------------------------------------------------------------ 5. / 6. the Forecaster
def _model(salt=0):
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(m, salt=salt)
    return m.to(DEV)


def _pal_obj(name="shanghai"):
    from adnm_hip.forecast import Palette
    return Palette(*_palette(name))


def _expect(res, fc):
    """.fields / .strip are the restatement applied to .pred"""
    edges, rgba = fc.palette.edges, fc.palette.colours
    p = res.pred.squeeze(2) if res.pred.dim() == 5 else res.pred
    wf, ws = R.render(_np(p), edges, rgba, fc.pixel_scale, fc.frame_start, fc.frame_step, fc.gap)
    assert tuple(res.fields.shape) == wf.shape and tuple(res.strip.shape) == ws.shape
    assert np.array_equal(_np(res.fields), wf) and np.array_equal(_np(res.strip), ws)
    return wf, ws


def test_forecaster_end_to_end(tmp_path):
    from adnm_hip.evaluator import GraphedForward
    from adnm_hip.forecast import Forecaster
    model = _model().eval()
    frames = recipe.radar_batch(2, 25, 64, name="radar64").to(DEV)           # the visionmamba_64_b2 fixture's parameters and input
    x1 = frames[:, :5].contiguous()
    x2 = recipe.radar_batch(2, 5, 64, name="forecast.other").to(DEV)
    fwd = GraphedForward(model)
    ref1, ref2 = fwd(x1).clone(), fwd(x2).clone()
    fwd.close()
    assert not torch.equal(ref1, ref2)
    # pixel_scale 255: the 64 x 64 model's output stays low, and a scale of 90 would leave most of the table unused
    fc = Forecaster(model, _pal_obj(), pixel_scale=255.0, frame_start=1, frame_step=2, gap=10)
    try:
        r1 = fc(x1)
        assert r1.pred.dtype == torch.float32 and torch.equal(r1.pred, ref1), "the Forecaster's forward is not GraphedForward's"
        assert tuple(r1.fields.shape) == (2, 20, 64, 64) and tuple(r1.strip.shape) == (2, 64, 10 * 64 + 9 * 10, 4) and fc.out_frames == 20
        f1, s1 = _expect(r1, fc)
        assert len(np.unique(f1)) >= 8, "the forecast is nearly constant: nothing is tested"
        r2 = fc(x2)
        assert torch.equal(r2.pred, ref2)
        f2, s2 = _expect(r2, fc)
        assert not np.array_equal(f1, f2) and not np.array_equal(s1, s2)
        assert r2.fields.data_ptr() == r1.fields.data_ptr(), "the results are the graph's static buffers"
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        r3 = fc(x1)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before, "a replay allocated"
        assert torch.equal(r3.pred, ref1) and np.array_equal(_np(r3.fields), f1) and np.array_equal(_np(r3.strip), s1)
        # the gt.png / input.png rows and the files
        gt = fc.render(frames[:, 5:])
        wf, ws = R.render(_np(frames[:, 5:].squeeze(2)), fc.palette.edges, fc.palette.colours, 255.0, 1, 2, 10)
        assert np.array_equal(_np(gt.fields), wf) and np.array_equal(_np(gt.strip), ws)
        inp = fc.render(x1, frame_start=0, frame_step=1)
        assert tuple(inp.strip.shape) == (2, 64, 5 * 64 + 4 * 10, 4)
        with pytest.raises(RuntimeError, match="built for"):
            fc.render(x1)                                                     # 5 frames under the forecast's 1::2 selection of 20
        paths = fc.save(str(tmp_path), r3, "ADNMUnet", batch=7)
        assert [p[len(str(tmp_path)):] for p in paths] == ["/7-1/ADNMUnet.png", "/7-2/ADNMUnet.png"]
        assert np.array_equal(R.decode_png(paths[1]), s1[1])
    finally:
        fc.close()
    fc.close()


def test_forecaster_raw_bytes():
    from adnm_hip import dataio
    from adnm_hip.forecast import Forecaster
    model = _model().eval()
    raw = torch.from_numpy(np.random.default_rng(11).integers(0, 71, size=(2, 5, 37, 53), dtype=np.uint8)).to(DEV)
    fc = Forecaster(model, _pal_obj(), pixel_scale=255.0, size=64, frame_start=1, frame_step=2)
    try:
        x = dataio.ingest(raw, 64)
        assert tuple(x.shape) == (2, 5, 1, 64, 64)
        a = fc(x)                                                             # the fp32-input graph
        pa, fa, sa = a.pred.clone(), a.fields.clone(), a.strip.clone()
        b = fc(raw)                                                           # the uint8-input graph: ingest in front of the forward
        assert b.fields.data_ptr() != a.fields.data_ptr() and len(fc._fwd._graphs) == 2
        assert torch.equal(b.pred, pa) and torch.equal(b.fields, fa) and torch.equal(b.strip, sa), "raw bytes and ingest() + fp32 differ"
        _expect(b, fc)
        raw2 = (raw // 2).contiguous()
        b2 = fc(raw2)
        a2 = fc(dataio.ingest(raw2, 64))
        assert torch.equal(b2.pred, a2.pred) and torch.equal(b2.strip, a2.strip) and not torch.equal(a2.pred, pa)
        with pytest.raises(RuntimeError, match="in_frames"):
            fc(raw[:, :4].contiguous())
    finally:
        fc.close()
    nosize = Forecaster(model, _pal_obj())
    with pytest.raises(RuntimeError, match="size="):
        nosize(raw)
    nosize.close()


# ------------------------------------------------------------------------------------------------ 7. beside a FlatTrainer
FP8_PERIOD = 2   # instead of 16: the record flags of the delayed-scaling table are SET while the second forecast runs


class _Precision:
    def __init__(self, prec):
        self.prec = prec

    def __enter__(self):
        self.period = ops.QUANT.period
        ops.QUANT.period = FP8_PERIOD
        ops.set_mfma_precision(self.prec)
        ops.QUANT.reset()

    def __exit__(self, *exc):
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()
        ops.QUANT.period = self.period
        return False


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)


def _same(a, b, what=""):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what} differs"
    elif isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), f"{what}: keys differ"
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        assert a == b, f"{what}: {a!r} vs {b!r}"


_data = {}


def _batches():
    if "b" not in _data:
        frames = recipe.radar_batch(8, 25, 64, name="forecast.train").to(DEV)
        _data["b"] = [(frames[i:i + 2, :5].contiguous(), frames[i:i + 2, 5:].contiguous()) for i in range(0, 8, 2)]
    return _data["b"]


def _train(forecast):
    """3 steps; forecast: a Forecaster call after step 1 and after step 2, and one after step 3 against the eager forward"""
    from adnm_hip.forecast import Forecaster
    from adnm_hip.trainer import FlatTrainer
    from models.loss import enRainfallLoss
    data = _batches()
    ops.QUANT.reset()
    model = _model().train()
    tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025, use_graph=True)
    fc = Forecaster(model, _pal_obj(), pixel_scale=255.0, frame_start=1, frame_step=2) if forecast else None
    preds, check = [], None
    try:
        for i in range(3):
            tr.step(*data[i])
            if forecast and i < 2:
                preds.append(fc(data[3][0]).pred.clone())
        state = tr.state_dict()
        params = {k: v.detach().to("cpu", copy=True) for k, v in model.state_dict().items()}
        if forecast:
            res = fc(data[3][0])                      # after step 3: it must have read the CURRENT narrow shadow
            _expect(res, fc)
            out = res.pred.clone()
            model.eval()
            with torch.no_grad():
                eager = model(data[3][0])
            model.train()
            torch.cuda.synchronize()
            check = (out, eager)
        return state, params, preds, check
    finally:
        if fc is not None:
            fc.close()
        tr.close()


@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_forecasting_beside_training(prec):
    with _Precision(prec):
        plain = _train(False)
        mixed = _train(True)
    _same(mixed[0], plain[0], "trainer state (moments, state, fp8: the quantisation table) after 3 steps with forecasts in between")
    _same(mixed[1], plain[1], "parameters after 3 steps with forecasts in between")
    if prec == "fp8":
        rows = plain[0]["fp8"]["rows"]
        assert len(rows) > 50 and bool((torch.stack([v[:2] for v in rows.values()]) != 1.0).any()), "no record ever made a scale: nothing is tested"
    p1, p2 = mixed[2]
    assert not torch.equal(p1, p2), "the second forecast saw the weights of the first: a stale shadow"
    out, eager = mixed[3]
    assert torch.equal(out, eager), "the Forecaster's forward after step 3 is not the eager forward on the current weights"


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals():
    from adnm_hip.forecast import Forecaster, Palette
    edges, rgba = _palette("shanghai")
    cpu = torch.zeros(2, 20, 16, 12)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.forecast_render(cpu, edges, rgba, 90.0)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.forecast_render(cpu.to(DEV).half(), edges, rgba, 90.0)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.forecast_render(cpu.to(DEV).to(torch.uint8), edges, rgba, 90.0)
    with pytest.raises(RuntimeError, match="fp32"):
        ops.forecast_render(cpu.to(DEV)[0], edges, rgba, 90.0)                    # (T, H, W): no batch dimension
    with pytest.raises(RuntimeError, match="neither"):
        ops.forecast_render(cpu.to(DEV), edges, rgba, 90.0, fields=False, strip=False)
    with pytest.raises(RuntimeError, match="1..32 bins"):                         # a palette of 33 colours, at the entry point
        ops.forecast_render(cpu.to(DEV), list(range(34)), np.zeros((33, 4), dtype=np.uint8), 90.0)
    with pytest.raises(ValueError, match="colours"):                              # ... and at the value type
        Palette(list(range(34)), np.zeros((33, 4), dtype=np.uint8))
    with pytest.raises(RuntimeError, match="palette"):
        ops.forecast_render(cpu.to(DEV), edges, rgba[:15], 90.0)
    with pytest.raises(RuntimeError, match="Palette"):
        Forecaster(torch.nn.Identity(), (edges, rgba))
    # an identity "model": the forecast is the input, T = 5
    fc = Forecaster(torch.nn.Identity(), Palette(edges, rgba), pixel_scale=90.0, frame_start=1, frame_step=2)
    x = torch.rand(2, 5, 1, 16, 12, device=DEV)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        fc(x.cpu())
    with pytest.raises(RuntimeError, match="fp32"):
        fc(x.half())
    with pytest.raises(RuntimeError, match="in_frames"):
        fc(x[:, :3].contiguous())
    res = fc(x)
    assert torch.equal(res.pred, x) and tuple(res.strip.shape) == (2, 16, 2 * 12 + 10, 4)
    _expect(res, fc)
    with pytest.raises(RuntimeError, match="built for the forecast's 5"):         # T different from what the frame selection was built for
        fc.render(torch.rand(2, 20, 16, 12, device=DEV))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        fc.render(x.cpu())
    fc.close()
    late = Forecaster(torch.nn.Identity(), Palette(edges, rgba), frame_start=7)   # refused on the warm-up forward's output, before any capture
    with pytest.raises(RuntimeError, match="frame_start 7"):
        late(x)
    assert not torch.cuda.is_current_stream_capturing()
    late.frame_start = 1                                                          # the refused call left nothing behind
    _expect(late(x), late)
    late.close()
