"""The long-interval (LAPS) recipe, create_ADNMUNet(5, 3, 60): GroupNorm, wavelet kernels [5,3,3], refine_dim [32,32,16,16].  On the CPU the
state_dict against the manifest recorded from the reference; on the GPU the whole model, the bf16 matrix-core mode and the FlatTrainer
against the fixtures the reference produced (tools/make_golden_groupnorm.py), with the checks and bars test_model_gpu.py and
test_trainer_gpu.py apply to the short-interval recipe."""
import json
import os

import pytest
import torch

from adnm_hip import recipe
from util import GOLDEN, load_npz, assert_close, check_update_deltas

gpu = pytest.mark.gpu
DEV = "cuda"
OUT_TOL = 1e-4
CIN, COUT, INTERVAL = 5, 3, 60


def make_model(size):
    from models.ADNMUNet import create_ADNMUNet
    model = create_ADNMUNet(CIN, COUT, INTERVAL, img_size=size)
    recipe.fill_parameters(model)
    return model


def test_laps_state_dict_matches_reference():
    with open(os.path.join(GOLDEN, "state_dict_manifest_laps.json")) as f:
        m = json.load(f)
    from models.ADNMUNet import create_ADNMUNet
    import torch.nn as nn
    model = create_ADNMUNet(CIN, COUT, INTERVAL)
    sd = model.state_dict()
    assert set(sd) == set(m), (sorted(set(sd) - set(m))[:5], sorted(set(m) - set(sd))[:5])
    assert list(sd) == list(m), "key order differs from the reference's"
    trainable = {k: p.requires_grad for k, p in model.named_parameters()}
    for k, v in sd.items():
        assert list(v.shape) == m[k]["shape"], k
        assert trainable[k] == m[k]["trainable"], k
        if m[k]["const"] is not None and k.split(".")[-1] != "bias":
            assert bool((v == m[k]["const"]).all()), f"{k}: init constant differs from the reference"
        if not m[k]["trainable"]:
            assert abs(float(v.double().sum()) - m[k]["sum"]) < 1e-9 * m[k]["abs"] + 1e-9, k
    norms = [mod for mod in model.modules() if isinstance(mod, (nn.GroupNorm, nn.InstanceNorm2d))]
    # PatchEmbed, 2 encoder + 3 decoder WTLayers, 7 EncoderToDecoders, OutProj
    assert len(norms) == 14 and all(isinstance(n, nn.GroupNorm) and (n.num_channels // n.num_groups) % 4 == 0 for n in norms)
    recipe.fill_parameters(model)
    for k, v in model.state_dict().items():
        if m[k]["trainable"]:
            assert abs(float(v.double().sum()) - m[k]["sum"]) <= 1e-6 * max(1.0, m[k]["abs"]), k


def test_laps_checkpoint_roundtrip(tmp_path):
    from adnm_hip import checkpoint
    a, b = make_model(64), make_model(64)
    with torch.no_grad():
        for p in b.parameters():
            if p.requires_grad:
                p.zero_()
    path = str(tmp_path / "ADNMUNet_laps.pth")
    n = checkpoint.save_reference_checkpoint(a, path, data_parallel_prefix=True)
    assert checkpoint.load_reference_checkpoint(b, path) == n == len(a.state_dict())
    assert any(k.endswith("norm.weight") for k in a.state_dict())
    for (k, v), (_, w) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(v, w), k


@gpu
@pytest.mark.parametrize("name,size,batch,radar", [("laps_64_b2", 64, 2, "laps64"), ("laps_128_b1", 128, 1, "laps128"),
                                                   ("laps_256_b1", 256, 1, "laps256")])
def test_laps_model_vs_reference(name, size, batch, radar):
    """as test_model_gpu.test_visionmamba_vs_reference"""
    from models.loss import enRainfallLoss
    z = load_npz(name)
    model = make_model(size).to(DEV).train()
    frames = recipe.radar_batch(batch, CIN + COUT, size, name=radar).to(DEV)
    x, tgt = frames[:, :CIN], frames[:, CIN:]
    taps = {}
    hooks = [model.encoder.register_forward_hook(lambda m, i, o: taps.__setitem__("encoder", o[0])),
             model.decoder.register_forward_hook(lambda m, i, o: taps.__setitem__("decoder", o)),
             model.refiner.refiner4.register_forward_hook(lambda m, i, o: taps.__setitem__("refiner4", o))]
    out = model(x)
    for h in hooks:
        h.remove()
    assert out.shape == (batch, COUT, 1, size, size)
    for k in ("encoder", "decoder", "refiner4"):
        assert_close(taps[k].flatten()[z[f"tap.{k}.idx"].to(DEV)], z[f"tap.{k}.val"], OUT_TOL, f"tap {k}")
    assert_close(out.flatten()[z["out_idx"].to(DEV)], z["out_samples"], OUT_TOL, "output samples")
    assert abs(float(out.double().norm()) - float(z["out_norm"])) <= OUT_TOL * float(z["out_norm"])
    if "out_full" in z:
        assert_close(out, z["out_full"], OUT_TOL, "full output")
    loss = enRainfallLoss(0.57, 0.25, gamma=0.0)(out, tgt)
    assert abs(float(loss) - float(z["loss"])) <= 1e-4 * abs(float(z["loss"]))
    loss.backward()
    names = [str(n) for n in z["names"]]
    gn, gtot = z["grad_norms"].numpy(), float(z["grad_total_norm"])
    named = dict(model.named_parameters())
    assert list(named) == names
    sq, nograd = 0.0, 0
    for i, k in enumerate(names):
        p = named[k]
        if gn[i] < 0:
            if p.requires_grad:
                nograd += 1
                assert p.grad is None, f"{k}: the reference leaves this parameter without a gradient"
            continue
        assert p.grad is not None, f"{k} has no gradient"
        n = float(p.grad.double().norm())
        sq += n * n
        assert abs(n - gn[i]) <= 2e-3 * gn[i] + 2e-4 * gtot, f"{k}: grad norm {n} vs {gn[i]}"
        pr = float((p.grad.double().flatten().cpu() * torch.from_numpy(recipe.sym("probe." + k, p.numel()))).sum())
        assert abs(pr - float(z["grad_probe"][i])) <= 5e-3 * gn[i] + 2e-4 * gtot, f"{k}: grad probe {pr} vs {float(z['grad_probe'][i])}"
    # the size of the no-gradient set is the reference's own, read from the fixture (it counts the frozen Haar filters too)
    frozen = sum(not p.requires_grad for p in named.values())
    assert nograd > 0 and nograd + frozen == int((gn < 0).sum()) == sum(p.grad is None for p in named.values())
    assert abs(sq ** 0.5 - gtot) <= 1e-3 * gtot
    before = [p.detach().double().clone() for p in model.parameters()]
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2)
    pre = torch.nn.utils.clip_grad_norm_(model.parameters(), 0.025)
    assert abs(float(pre) - float(z["clip_pre_norm"])) <= 1e-3 * float(z["clip_pre_norm"])
    opt.step()
    ref_sums = z["param_sum_after_step"].numpy()
    for i, k in enumerate(names):
        s = float(named[k].double().sum())
        assert abs(s - ref_sums[i]) <= 2.5e-3 * named[k].numel() ** 0.5 + 1e-5 * abs(ref_sums[i]) + 1e-6, k
    check_update_deltas(z, names, [p.detach().double() - b for p, b in zip(model.parameters(), before)])


@gpu
def test_laps_bf16_mfma_vs_reference():
    """as test_model_gpu.test_visionmamba_bf16_mfma_vs_reference: 6e-2 vs the reference's fp32 outputs, 3e-2 vs this build's fp32 path, loss
    within 2 %, total gradient norm within 5 %"""
    from adnm_hip import ops
    from models.loss import enRainfallLoss
    z = load_npz("laps_64_b2")
    model = make_model(64).to(DEV).train()
    frames = recipe.radar_batch(2, CIN + COUT, 64, name="laps64").to(DEV)
    x, tgt = frames[:, :CIN], frames[:, CIN:]
    with torch.no_grad():
        y32 = model(x)
    ops.set_mfma_precision("bf16")
    try:
        out = model(x)
        loss = enRainfallLoss(0.57, 0.25, gamma=0.0)(out, tgt)
        loss.backward()
    finally:
        ops.set_mfma_precision("f32")
    assert_close(out.flatten()[z["out_idx"].to(DEV)], z["out_samples"], 6e-2, "bf16 output samples vs the reference (fp32)")
    assert_close(out, y32, 3e-2, "bf16 vs this build's fp32 path")
    assert float((out - y32).abs().max()) > 0.0
    assert abs(float(loss) - float(z["loss"])) <= 2e-2 * abs(float(z["loss"]))
    total = sum(float(p.grad.double().pow(2).sum()) for p in model.parameters() if p.grad is not None) ** 0.5
    assert abs(total - float(z["grad_total_norm"])) <= 5e-2 * float(z["grad_total_norm"])


@gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_laps_trainer_step_vs_reference_fixture(use_graph):
    """as test_trainer_gpu.test_whole_model_step_vs_reference_fixture: the GroupNorm weights and biases are ordinary fp32 members of the
    flat buffers (born-in-place gradients through the deferred fold, fused clip + AdamW, graph replay)"""
    from adnm_hip.trainer import FlatTrainer
    from models.loss import enRainfallLoss
    z = load_npz("laps_64_b2")
    model = make_model(64).to(DEV).train()
    frames = recipe.radar_batch(2, CIN + COUT, 64, name="laps64").to(DEV)
    x, tgt = frames[:, :CIN], frames[:, CIN:]
    tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                     use_graph=use_graph)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    loss = tr.step(x, tgt)
    assert abs(float(loss) - float(z["loss"])) <= 1e-4 * abs(float(z["loss"]))
    assert abs(float(tr.grad_norm()) - float(z["clip_pre_norm"])) <= 1e-3 * float(z["clip_pre_norm"])
    names, ref_sums, gn = [str(n) for n in z["names"]], z["param_sum_after_step"].numpy(), z["grad_norms"].numpy()
    named = dict(model.named_parameters())
    for i, k in enumerate(names):
        p = named[k]
        s = float(p.double().sum())
        assert abs(s - ref_sums[i]) <= 2.5e-3 * p.numel() ** 0.5 + 1e-5 * abs(ref_sums[i]) + 1e-6, k
        if gn[i] < 0:
            assert torch.equal(p, before[k]), k
    check_update_deltas(z, names, [named[k].detach().double() - before[k].double() for k in names])
    tr.close()


@gpu
def test_laps_graphed_eval_forward_matches_eager():
    from adnm_hip.evaluator import GraphedForward
    model = make_model(64).to(DEV).eval()
    fwd = GraphedForward(model)
    for salt in (0, 1):
        x = recipe.radar_batch(2, CIN, 64, salt=salt, name="lapsfwd").to(DEV)
        with torch.no_grad():
            ref = model(x)
        out = fwd(x)
        assert out.shape == (2, COUT, 1, 64, 64) and not out.requires_grad
        assert torch.equal(out, ref)
