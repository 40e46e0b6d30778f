"""The HIP GroupNorm (adnm_groupnorm_fwd / _bwd through ops.groupnorm): the C-ABI surface on the CPU; on the GPU the kernels against
float64 torch (F.group_norm + the layer's scalar affine + GELU, through autograd), bitwise repeatability of the parameter gradients,
the fold queue, the support rule at the three norm sites, and the InstanceNorm=False module fixtures recorded from the reference
(tools/make_golden_groupnorm.py).  Tolerances: those of test_kernels_gpu.test_instnorm and test_model_gpu."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from adnm_hip import ops, lib, recipe
from util import load_case, assert_close, rel_l2

gpu = pytest.mark.gpu
DEV = "cuda"
OUT_TOL, GRAD_TOL, GRAD_ATOL = 1e-4, 1e-3, 2e-5


def T(name, shape, scale=1.0):
    return recipe.tensor(name, shape, scale)


def leaf(t, dev=None):
    t = t.clone().to(dev) if dev else t.clone()
    return t.requires_grad_(True)


# ------------------------------------------------------------------------------------------- C-ABI (no GPU needed)
def test_header_declares_and_library_exports_groupnorm():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ("adnm_groupnorm_ws_bytes", "adnm_groupnorm_fwd", "adnm_groupnorm_bwd"):
        assert name in protos, f"{name} not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} not exported"
    assert lib.load().adnm_abi_version() == 11   # (GroupNorm itself was purely additive)


def test_groupnorm_ws_query_is_a_pure_host_function():
    assert lib.query("adnm_groupnorm_ws_bytes", 4, 16384, 32, 4) > 0


def test_groupnorm_rejects_partial_quads_per_group_before_any_launch():
    rc = lib.load().adnm_groupnorm_fwd(1, None, None, None, None, 1, 1, 1, 1, 1 << 20, 1, 16, 8, 4, 1e-5, 0, 0, None)
    assert rc == -1 and "multiple of 4 channels per group" in lib.last_error(), lib.last_error()
    rc = lib.load().adnm_groupnorm_bwd(1, 1, None, None, None, None, 1, 1, 1, None, None, None, None, 1, 1 << 20, 1, 16, 8, 4, 0, 0, None)
    assert rc == -1 and "multiple of 4 channels per group" in lib.last_error(), lib.last_error()
    rc = lib.load().adnm_groupnorm_fwd(1, None, None, None, None, 1, 1, 1, 1, 1 << 20, 1, 16, 24, 5, 1e-5, 0, 0, None)
    assert rc == -1 and "do not divide" in lib.last_error(), lib.last_error()


# ------------------------------------------------------------------------------------------- kernels vs float64 torch
SHAPES = [(4, 16384, 32, 4), (4, 16384, 64, 8),   # the full-resolution sites of the 128 x 128, B = 4 workload
          (2, 1024, 128, 4),
          (2, 16, 1024, 4),                        # deep level: one group = 256 channels, 16 pixels
          (3, 77, 16, 4),                          # ragged pixel count, 4 channels per group (OutProj)
          (2, 40, 528, 4)]                         # 33 quads per group: groups straddle the 64-quad workgroups (merged from global partials)


def make_inputs(B, HW, C, common=0.0):
    """test_instnorm's inputs (spread 2, per-channel offsets of 1.5 x the spread), plus an offset common to all channels"""
    x = T("gn.x", (B, HW, C), 2.0) + 3.0 * T("gn.m", (1, 1, C)) + common
    return x, T("gn.c", (B, HW, C)), 1 + 0.2 * T("gn.g", (C,)), 0.3 * T("gn.b", (C,)), torch.tensor(0.9), torch.tensor(0.15)


def torch_chain(x, G, w, b, sc, sh, act, eps=1e-5):
    y = F.group_norm(x.transpose(1, 2), G, w, b, eps).transpose(1, 2)
    y = sc * y + sh
    return F.gelu(y) if act == lib.ACT_GELU else y


def run_kernel(x, cot, G, w, b, sc, sh, act, dtype=torch.float32):
    xg = leaf(x.to(dtype), DEV)
    wg, bg = (leaf(w, DEV), leaf(b, DEV)) if w is not None else (None, None)
    scg, shg = leaf(sc, DEV), leaf(sh, DEV)
    yg = ops.groupnorm(xg, G, wg, bg, scg, shg, 1e-5, act)
    (yg * cot.to(DEV).to(dtype)).sum().backward()
    return yg, xg, wg, bg, scg, shg


@gpu
@pytest.mark.parametrize("act", [lib.ACT_NONE, lib.ACT_GELU])
@pytest.mark.parametrize("B,HW,C,G", SHAPES)
def test_groupnorm_vs_float64(B, HW, C, G, act):
    x, cot, w, b, sc, sh = make_inputs(B, HW, C)
    xo, wo, bo, sco, sho = (leaf(t.double()) for t in (x, w, b, sc, sh))
    yo = torch_chain(xo, G, wo, bo, sco, sho, act)
    (yo * cot.double()).sum().backward()
    yg, xg, wg, bg, scg, shg = run_kernel(x, cot, G, w, b, sc, sh, act)
    print(f"groupnorm {B}x{HW}x{C}/{G} act {act}: y {rel_l2(yg.cpu(), yo):.2e} dx {rel_l2(xg.grad.cpu(), xo.grad):.2e} "
          f"dgamma {rel_l2(wg.grad.cpu(), wo.grad):.2e} dbeta {rel_l2(bg.grad.cpu(), bo.grad):.2e} "
          f"dscale {rel_l2(scg.grad.cpu(), sco.grad):.2e} dshift {rel_l2(shg.grad.cpu(), sho.grad):.2e}")
    assert_close(yg, yo, OUT_TOL, "y")
    assert_close(xg.grad, xo.grad, GRAD_TOL, "dx", atol=1e-7)
    assert_close(wg.grad, wo.grad, GRAD_TOL, "dgamma")
    assert_close(bg.grad, bo.grad, GRAD_TOL, "dbeta")
    assert_close(scg.grad, sco.grad, GRAD_TOL, "dscale", atol=1e-4)
    assert_close(shg.grad, sho.grad, GRAD_TOL, "dshift", atol=1e-4)


@gpu
@pytest.mark.parametrize("B,HW,C,G", [(4, 16384, 32, 4), (2, 16, 1024, 4)])
def test_groupnorm_large_common_offset(B, HW, C, G):
    """All channels offset by 100 x the spread: a variance from unshifted (or wrongly merged shifted) sums cancels here.  The fp32 input
    itself carries ~100 x 2^-24 of relative round-off, so the bar on y is not OUT_TOL but 4 x the error of torch's own fp32
    F.group_norm chain on the same input against float64, computed here; the gradient bars are the usual ones."""
    act = lib.ACT_GELU
    x, cot, w, b, sc, sh = make_inputs(B, HW, C, common=200.0)
    xo, wo, bo, sco, sho = (leaf(t.double()) for t in (x, w, b, sc, sh))
    yo = torch_chain(xo, G, wo, bo, sco, sho, act)
    (yo * cot.double()).sum().backward()
    bar = 4 * rel_l2(torch_chain(x, G, w, b, sc, sh, act), yo)
    yg, xg, wg, bg, scg, shg = run_kernel(x, cot, G, w, b, sc, sh, act)
    print(f"groupnorm +100 spreads {B}x{HW}x{C}/{G}: y {rel_l2(yg.cpu(), yo):.2e} (bar {bar:.2e}) dx {rel_l2(xg.grad.cpu(), xo.grad):.2e} "
          f"dgamma {rel_l2(wg.grad.cpu(), wo.grad):.2e} dbeta {rel_l2(bg.grad.cpu(), bo.grad):.2e}")
    assert_close(yg, yo, bar, "y")
    assert_close(xg.grad, xo.grad, GRAD_TOL, "dx", atol=1e-7)
    assert_close(wg.grad, wo.grad, GRAD_TOL, "dgamma")
    assert_close(bg.grad, bo.grad, GRAD_TOL, "dbeta")
    assert_close(scg.grad, sco.grad, GRAD_TOL, "dscale", atol=1e-4)
    assert_close(shg.grad, sho.grad, GRAD_TOL, "dshift", atol=1e-4)


@gpu
@pytest.mark.parametrize("B,HW,C,G", SHAPES)
def test_groupnorm_bf16_storage(B, HW, C, G):
    """bf16 activations in and out (statistics, parameters and workspace stay fp32): 2e-2 on y, the bar of test_bf16_storage_paths"""
    x, cot, w, b, sc, sh = make_inputs(B, HW, C)
    with torch.no_grad():
        yo = torch_chain(x.double(), G, w.double(), b.double(), sc.double(), sh.double(), lib.ACT_GELU)
    yg, xg, wg, bg, scg, shg = run_kernel(x, cot, G, w, b, sc, sh, lib.ACT_GELU, dtype=torch.bfloat16)
    assert yg.dtype == torch.bfloat16 and xg.grad.dtype == torch.bfloat16 and wg.grad.dtype == torch.float32
    print(f"groupnorm bf16 {B}x{HW}x{C}/{G}: y {rel_l2(yg.float().cpu(), yo):.2e}")
    assert_close(yg.float(), yo, 2e-2, "bf16 y")
    assert bool(torch.isfinite(xg.grad.float()).all()) and bool(torch.isfinite(wg.grad).all())


@gpu
def test_groupnorm_without_affine():
    """GroupNorm(4, 16, affine=False): NULL gamma / beta"""
    B, HW, C, G = 3, 77, 16, 4
    x, cot, _, _, sc, sh = make_inputs(B, HW, C)
    xo, sco, sho = leaf(x.double()), leaf(sc.double()), leaf(sh.double())
    yo = torch_chain(xo, G, None, None, sco, sho, lib.ACT_GELU)
    (yo * cot.double()).sum().backward()
    yg, xg, _, _, scg, shg = run_kernel(x, cot, G, None, None, sc, sh, lib.ACT_GELU)
    assert_close(yg, yo, OUT_TOL, "y")
    assert_close(xg.grad, xo.grad, GRAD_TOL, "dx", atol=1e-7)
    assert_close(scg.grad, sco.grad, GRAD_TOL, "dscale", atol=1e-4)
    assert_close(shg.grad, sho.grad, GRAD_TOL, "dshift", atol=1e-4)
    from models.model_untils import WTConvLayer
    layer = WTConvLayer(16, 16, kernel_size=3, wt_levels=1, norm=nn.GroupNorm(4, 16, affine=False), act_func=nn.GELU).to(DEV)
    y = layer.forward_tokens(T("gn.na", (1, 64, 16)).to(DEV), 8, 8)
    assert y.shape == (1, 64, 16) and bool(torch.isfinite(y).all())


@gpu
@pytest.mark.parametrize("B,HW,C,G", [(4, 16384, 32, 4), (2, 16, 1024, 4), (2, 40, 528, 4)])
def test_groupnorm_parameter_gradients_are_bitwise_repeatable(B, HW, C, G):
    """no float atomics: two identical backward calls agree bit for bit, and so do the immediate and the queued (deferred) fold"""
    x, cot, w, b, sc, sh = make_inputs(B, HW, C)
    grads = []
    for defer in (False, False, True):
        if defer:
            ops.FOLDS.enable(torch.device(DEV, torch.cuda.current_device()), False)   # creates the device's queue; off outside the scope below
            with ops.FOLDS.active(torch.device(DEV, torch.cuda.current_device())):
                r = run_kernel(x, cot, G, w, b, sc, sh, lib.ACT_GELU)
        else:
            r = run_kernel(x, cot, G, w, b, sc, sh, lib.ACT_GELU)
        torch.cuda.synchronize()
        grads.append([t.grad.clone() for t in r[1:]])
    for other, what in ((grads[1], "second call"), (grads[2], "fold queue bound")):
        for a, o, name in zip(grads[0], other, ("dx", "dgamma", "dbeta", "dscale", "dshift")):
            assert torch.equal(a, o), f"{name}: {what} differs"


@gpu
def test_groupnorm_support_rule_at_the_norm_sites():
    from models.model_untils import Conv2dLayer, WTConvLayer, EncoderToDecoder
    tok = torch.zeros(1, 16, 8, device=DEV)
    with pytest.raises(RuntimeError, match="no PyTorch fallback"):       # two channels per group
        Conv2dLayer(8, 8, norm=nn.GroupNorm(4, 8)).to(DEV).forward_tokens(tok, 4, 4)
    with pytest.raises(RuntimeError, match="no PyTorch fallback"):
        WTConvLayer(8, 8, kernel_size=5, wt_levels=1, norm=nn.GroupNorm(4, 8)).to(DEV).forward_tokens(tok, 4, 4)
    with pytest.raises(RuntimeError, match="no PyTorch fallback"):
        EncoderToDecoder(embed_dim=8, InstanceNorm=False).to(DEV)(tok, torch.zeros(1, 1, 8, device=DEV))
    with pytest.raises(RuntimeError, match="multiple of 4 channels per group"):   # the op itself: rejected by the library, nothing launched
        ops.groupnorm(tok, 4)
    # a supported GroupNorm behind a pointwise conv: Conv2dLayer's site, against torch on the same weights
    layer = Conv2dLayer(8, 16, kernel_size=(1, 1), padding=(0, 0), norm=nn.GroupNorm(2, 16), act_func=nn.GELU).to(DEV)
    recipe.fill_parameters(layer)
    x = T("gn.site", (2, 36, 8)).to(DEV)
    y = layer.forward_tokens(x, 6, 6)
    with torch.no_grad():
        z = F.conv2d(x.double().transpose(1, 2).reshape(2, 8, 6, 6), layer.conv.weight.double(), None if layer.conv.bias is None else layer.conv.bias.double())
        z = F.gelu(layer.scale.double() * F.group_norm(z, 2, layer.norm.weight.double(), layer.norm.bias.double(), layer.norm.eps) + layer.shift.double())
    assert_close(y, z.reshape(2, 16, 36).transpose(1, 2), OUT_TOL, "Conv2dLayer + GroupNorm")


# ------------------------------------------------------------------------------------------- module fixtures from the reference
def run_case(name, build, call, grad_inputs):
    """as tests/test_model_gpu.py run_case"""
    params, grads, ins, gins, outs, cots = load_case(name)
    mod = build()
    mod.load_state_dict(params, strict=True)
    mod = mod.to(DEV)
    xin = {k: v.to(DEV).requires_grad_(k in grad_inputs) for k, v in ins.items()}
    got = call(mod, **xin)
    got = got if isinstance(got, (tuple, list)) else (got,)
    loss = 0
    for i, (g, o, c) in enumerate(zip(got, outs, cots)):
        assert_close(g.reshape(o.shape), o, OUT_TOL, f"{name} out{i}")
        loss = loss + (g.reshape(o.shape) * c.to(DEV)).sum()
    loss.backward()
    for k in grad_inputs:
        assert_close(xin[k].grad, gins[k], GRAD_TOL, f"{name} d{k}", GRAD_ATOL)
    named = dict(mod.named_parameters())
    assert any(k.endswith("norm.weight") for k in grads), f"{name}: the fixture carries no GroupNorm weight gradient"
    for k, g in grads.items():
        assert named[k].grad is not None, f"{name}: no grad for {k}"
        assert_close(named[k].grad, g, GRAD_TOL, f"{name} d{k}", GRAD_ATOL)
    for k, p in named.items():
        if k not in grads and p.requires_grad:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, f"{name}: {k} must not receive a gradient"


@gpu
def test_groupnorm_modules_vs_reference_fixtures():
    from models import model_untils as U
    run_case("gn_patch_embed_5_16", lambda: U.PatchEmbed(img_size=16, patch_size=2, in_channels=5, embed_dim=16, kernel=5, wt_levels=3,
                                                         InstanceNorm=False), lambda m, x: m(x), ("x",))
    run_case("gn_wtlayer_16_24", lambda: U.WTLayer(16, 24, kernel=5, wt_levels=2, InstanceNorm=False), lambda m, x: m(x), ("x",))
    run_case("gn_wtlayer_res_32_16", lambda: U.WTLayer(32, 16, kernel=3, wt_levels=1, if_res=True, InstanceNorm=False),
             lambda m, x, r, f: m(x, residual=r, features=f), ("x", "r"))
    run_case("gn_e2d_16", lambda: U.EncoderToDecoder(embed_dim=16, InstanceNorm=False), lambda m, x, res: m(x, res), ("x", "res"))
    run_case("gn_outproj_16_3", lambda: U.OutProj(num_frames=3, embed_dim=16, img_size=[16, 16], wt_levels=3, out_expand=2, InstanceNorm=False),
             lambda m, x, res: m(x, res), ("x",))
