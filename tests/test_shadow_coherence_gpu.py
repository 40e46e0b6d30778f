"""The narrow weight SHADOW of a prepared FlatTrainer (ops.ShadowSet: bf16 / scaled e4m3 copy of the flat parameter buffer that the
weight-streaming GEMMs read instead of the fp32 values) after writes made OUTSIDE the optimiser: load_state_dict, the reference-checkpoint
loader, in-place ops, writes torch cannot see.  Every later eager forward, GraphedForward replay and training step must compute with the
NEW weights: bit for bit what a model holding them with ADNM_NARROW_WEIGHTS=0 (fp32 weights rounded on the fly) computes in bf16, and in
fp8 with weight scales re-derived from the new weights.  A GraphedForward that outlives its trainer keeps the shadow it reads alive.
W' (salt 1 of recipe.fill_parameters) gives outputs unrelated to salt 0, so a stale shadow cannot pass by accident."""
import gc
import weakref

import pytest
import torch

from adnm_hip import ops, recipe
from adnm_hip.trainer import FlatTrainer
from util import _e4m3_bytes, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
# deep-level weights of the short GEMMs (k_linear on the shadow): the in-place test writes the first that exists
INPLACE_CANDIDATES = ("encoder.encoder6.out_proj.weight", "encoder.attn2.attn_mlp.fc2.weight", "decoder.decoder1.out_proj.weight")


def _model(salt=0, size=64):
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=size)
    recipe.fill_parameters(m, salt=salt)
    return m.to(DEV).train()


def _state(salt=1, size=64):
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=size)
    recipe.fill_parameters(m, salt=salt)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _batch(b=2, size=64, name="coherence"):
    frames = recipe.radar_batch(b, 25, size, name=name).to(DEV)
    return frames[:, :5].contiguous(), frames[:, 5:].contiguous()


def _trainer(model):
    from models.loss import enRainfallLoss
    return FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, max_norm=0.025, use_graph=True)


def _trained(x, tgt, steps=2, size=64):
    model = _model(0, size)
    tr = _trainer(model)
    for _ in range(steps):
        tr.step(x, tgt)
    return model, tr


def _reference_forward(monkeypatch, sd, x, tgt):
    """eval forward of a model holding `sd` in the trainer's flat layout, WITHOUT a shadow (ADNM_NARROW_WEIGHTS=0: the fp32 weights
    rounded on the way into the matrix cores), at the current precision"""
    with monkeypatch.context() as mp:
        mp.setenv("ADNM_NARROW_WEIGHTS", "0")
        model = _model(0, x.shape[-1])
        model.load_state_dict(sd)
        tr = FlatTrainer(model, _loss(), lr=1e-3, max_norm=0.025, use_graph=False)
        tr.prepare(x, tgt)   # (flattens; no optimiser step)
        assert tr.shadow is None
        tr.close()
        model.eval()
        with torch.no_grad():
            out = model(x).clone()
    torch.cuda.synchronize()
    return out


def _loss():
    from models.loss import enRainfallLoss
    return enRainfallLoss(0.57, 0.25, gamma=0.0)


def _eval(model, x):
    model.eval()
    with torch.no_grad():
        out = model(x).clone()
    model.train()
    return out


def _quant_tab(dev):
    """the device's fp8 record table: [scale_a, scale_b, amax_a, amax_b, fmax_a, fmax_b, record, -] per row"""
    return ops.QUANT._ent(torch.device(dev))["tab"]


def _pins(dev):
    return ops.QUANT._ent(torch.device(dev)).get("pins", 0)


def _cpu_state(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


@pytest.fixture
def bf16():
    ops.set_mfma_precision("bf16")
    try:
        yield
    finally:
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()


@pytest.fixture
def fp8():
    ops.set_mfma_precision("fp8")
    try:
        yield
    finally:
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()


# ------------------------------------------------------------------ bf16
def test_bf16_eval_after_load_state_dict(bf16, monkeypatch):
    x, tgt = _batch()
    model, tr = _trained(x, tgt)
    try:
        assert tr.shadow_mode == 1
        w1 = _state(1)
        model.load_state_dict(w1)
        out = _eval(model, x)
    finally:
        tr.close()
    ref = _reference_forward(monkeypatch, w1, x, tgt)
    assert torch.equal(out, ref), f"eval forward after load_state_dict reads stale weights (rel-L2 {rel_l2(out, ref):.3e})"


def test_bf16_eval_after_reference_checkpoint(bf16, monkeypatch, tmp_path):
    from adnm_hip.checkpoint import load_reference_checkpoint, save_reference_checkpoint
    x, tgt = _batch()
    donor = _model(1)
    path = str(tmp_path / "ADNMUNet_best.pth")
    save_reference_checkpoint(donor, path, data_parallel_prefix=True)
    w1 = _cpu_state(donor)
    del donor
    model, tr = _trained(x, tgt)
    try:
        assert load_reference_checkpoint(model, path) == len(w1)
        out = _eval(model, x)
    finally:
        tr.close()
    ref = _reference_forward(monkeypatch, w1, x, tgt)
    assert torch.equal(out, ref), f"eval forward after load_reference_checkpoint reads stale weights (rel-L2 {rel_l2(out, ref):.3e})"


def test_bf16_graphed_eval_after_load(bf16, monkeypatch):
    from adnm_hip.evaluator import GraphedForward
    x, tgt = _batch()
    w1 = _state(1)
    ref = _reference_forward(monkeypatch, w1, x, tgt)
    model, tr = _trained(x, tgt)
    try:
        fwd = GraphedForward(model)
        before = fwd(x).clone()   # captured while training
        tr.step(x, tgt)
        model.load_state_dict(w1)
        out = fwd(x).clone()
        torch.cuda.synchronize()
        assert not torch.equal(before, ref)
        assert torch.equal(out, ref), f"GraphedForward replay after load reads a stale shadow (rel-L2 {rel_l2(out, ref):.3e})"
        fwd.close()
    finally:
        tr.close()


def test_bf16_training_step_after_load(bf16, monkeypatch):
    x, tgt = _batch()
    model, tr = _trained(x, tgt)
    try:
        w1 = _state(1)
        model.load_state_dict(w1)
        loss = float(tr.step(x, tgt))
        torch.cuda.synchronize()
        g = tr.flat_g.clone()
        assert torch.equal(tr.shadow, tr.flat_p.to(torch.bfloat16)), "the shadow is bf16(p) after the step"
    finally:
        tr.close()
    with monkeypatch.context() as mp:
        mp.setenv("ADNM_NARROW_WEIGHTS", "0")
        ref_model = _model(0)
        ref_model.load_state_dict(w1)
        ref = _trainer(ref_model)
        try:
            ref_loss = float(ref.step(x, tgt))
            torch.cuda.synchronize()
            assert ref.shadow is None and ref.n == g.numel()
            ref_g = ref.flat_g.clone()
        finally:
            ref.close()
    assert loss == ref_loss, f"loss after load {loss!r} vs a fresh trainer on the loaded weights {ref_loss!r}"
    assert torch.equal(g, ref_g), f"gradients after load differ from a fresh trainer's (rel-L2 {rel_l2(g, ref_g):.3e})"


def test_bf16_in_place_writes(bf16, monkeypatch):
    x, tgt = _batch()
    model, tr = _trained(x, tgt)
    try:
        named = dict(model.named_parameters())
        name = next(n for n in INPLACE_CANDIDATES if n in named and any(named[n] is q for q in tr.used))
        p = named[name]
        assert ops.SHADOWS.lookup(p, 1) is not None, f"{name} must be read through the shadow"
        before = _eval(model, x)
        # (1) an in-place torch op: detected through the parameter's version counter
        with torch.no_grad():
            p.mul_(0.5)
        out1 = _eval(model, x)
        sd1 = _cpu_state(model)
        # (2) a write torch cannot see (p.data is a new alias with its own counter): needs refresh_shadows()
        p.data.copy_(p.data * -3.0)
        tr.refresh_shadows()
        out2 = _eval(model, x)
        sd2 = _cpu_state(model)
    finally:
        tr.close()
    ref1 = _reference_forward(monkeypatch, sd1, x, tgt)
    ref2 = _reference_forward(monkeypatch, sd2, x, tgt)
    assert not torch.equal(before, ref1), f"{name}: halving it must change the output"
    assert torch.equal(out1, ref1), f"forward after p.mul_(0.5) on {name} reads a stale shadow (rel-L2 {rel_l2(out1, ref1):.3e})"
    assert torch.equal(out2, ref2), f"forward after p.data.copy_ + refresh_shadows() on {name} (rel-L2 {rel_l2(out2, ref2):.3e})"


# ------------------------------------------------------------------ fp8
def test_fp8_weight_records_after_load(fp8):
    x, tgt = _batch()
    model, tr = _trained(x, tgt)
    try:
        assert tr.shadow_mode == 2
        names = {id(p): n for n, p in model.named_parameters()}
        rows = tr.seg_rec.tolist()
        recs = [(i, names[id(p)], rows[i]) for i, p in enumerate(tr.used) if rows[i] >= 0]
        assert len(recs) > 50
        w2 = _state(1)
        for _, n, _ in recs:   # x4: the old scales would saturate every one of them at 448
            w2[n] = w2[n] * 4.0
        old = _quant_tab(x.device)[:, 1].clone()
        model.load_state_dict(w2)
        _eval(model, x)   # the eager lookups rewrite the stale shadow (and the weight scales) before the first read
        torch.cuda.synchronize()
        tab = _quant_tab(x.device).cpu()
        hr = torch.tensor(ops.QUANT.headroom, dtype=torch.float32)
        for i, n, r in recs:
            amax = w2[n].float().abs().max()
            want = torch.tensor(448.0, dtype=torch.float32) / (amax * hr)
            got = tab[r, 1]
            assert float(got) == float(want), f"{n}: scale_b {float(got)!r}, want 448 / (amax * headroom) = {float(want)!r} (was {float(old[r])!r})"
            assert float(got) != float(old[r]), f"{n}: scale_b unchanged by a x4 load"
            o, k = tr.offs[i], tr.used[i].numel()
            assert torch.equal(tr.shadow[o:o + k], _e4m3_bytes(tr.flat_p[o:o + k] * got.to(DEV))), f"{n}: fp8 shadow bytes"
    finally:
        tr.close()


def test_fp8_eval_forward_after_load(fp8):
    """At the shape of the fp8 bars (128x128, B = 4, batch "bench").  W' itself is harder for e4m3 than the salt-0 parameters that
    test_visionmamba_fp8_vs_reference measures (measured: 0.20 rel-L2 against fp32 with a fresh calibration of every record, 0.10 at
    salt 0), so the bar is what a fresh fp8 calibration on W' reaches, measured here first, with 10 % to spare; a stale shadow or
    stale weight scales land far outside it."""
    x, tgt = _batch(4, 128, "bench")
    w1 = _state(1, 128)
    ops.set_mfma_precision("f32")
    ref_model = _model(0, 128)
    ref_model.load_state_dict(w1)
    ref_model.eval()
    with torch.no_grad():
        y32 = ref_model(x).clone()
        ops.fp8_calibrate(x.device, lambda: ref_model(x))   # every record from this forward; leaves the precision at fp8
        y8 = ref_model(x).clone()
    del ref_model
    ops.QUANT.reset()
    bar = rel_l2(y8, y32)
    model, tr = _trained(x, tgt, size=128)
    try:
        model.load_state_dict(w1)
        out = _eval(model, x)
    finally:
        tr.close()
    err = rel_l2(out, y32)
    print(f"fp8 eval forward after load: rel-L2 vs the fp32 forward of the loaded weights {err:.3e} "
          f"(a fresh fp8 calibration on them: {bar:.3e})")
    assert float((out - y32).abs().max()) > 0.0, "the fp8 path must differ from fp32"
    assert err <= 1.1 * bar and err <= 0.25, f"fp8 eval forward after load: rel-L2 {err:.3e} vs fp32 (fresh calibration {bar:.3e})"


# ------------------------------------------------------------------ lifetime
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_graphed_forward_outlives_its_trainer(prec, monkeypatch):
    from adnm_hip.evaluator import GraphedForward
    x, tgt = _batch()
    ops.set_mfma_precision(prec)
    try:
        model, tr = _trained(x, tgt)
        pins0 = _pins(x.device)
        fwd = GraphedForward(model)
        first = fwd(x).clone()
        assert _pins(x.device) == pins0 + (prec == "fp8")
        sd = _cpu_state(model)
        alive = weakref.ref(tr.shadow)
        tr.close()
        del tr
        gc.collect()
        assert alive() is not None, "the captured graph reads the shadow: the GraphedForward must keep it alive"
        out = fwd(x).clone()   # (only replayed with the shadow alive)
        torch.cuda.synchronize()
        assert torch.equal(out, first), "replay after the trainer closed"
        if prec == "bf16":
            ref = _reference_forward(monkeypatch, sd, x, tgt)
            assert torch.equal(out, ref), f"replay after the trainer closed vs the reference (rel-L2 {rel_l2(out, ref):.3e})"
        fwd.close()
        fwd.close()   # idempotent
        gc.collect()
        assert alive() is None, "fwd.close() must let the shadow go"
        # the trainer's own pin went with tr.close(); the GraphedForward's with fwd.close()
        assert _pins(x.device) == pins0 - (prec == "fp8")
    finally:
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()
