"""Level 0 of WTConv2d fused with the module's base depthwise conv (adnm_wt_level_base): bitwise against the launches it replaces —
the level kernel + the depthwise kernel on the same operands — and, for the whole autograd node, against the node composed from those
primitives the way ops.WTConvFn ran them before the fusion."""
import pytest
import torch

from adnm_hip import ops, lib, recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(name, shape, scale=1.0):
    return recipe.tensor(name, shape, scale).to(DEV)


# (B, H, W, C, K, bias)
CASES = [
    (2, 16, 16, 8, 5, True),       # baseline
    (1, 11, 13, 4, 3, False),      # odd sizes, K = 3, channel block 4
    (2, 20, 28, 8, 5, False),      # partial tiles
    (1, 5, 7, 12, 5, True),        # map smaller than one tile
    (4, 64, 64, 128, 5, False),    # >= 256 workgroups at the widest channel block (8 MB)
]


@pytest.mark.parametrize("B,H,W,C,K,bias", CASES)
@pytest.mark.parametrize("flip", [False, True], ids=["fwd", "bwd"])
def test_wt_level_base_bitwise(B, H, W, C, K, bias, flip):
    tag_ = f"wtf.{B}.{H}.{W}.{C}.{K}"
    x = T(tag_ + ".x", (B * H * W, C))
    taps = T(tag_ + ".t", (K * K, 4 * C), 0.3)
    bw = T(tag_ + ".bw", (K * K, C), 0.3)
    bb = T(tag_ + ".bb", (C,), 0.3) if bias else None
    sub0, tag0 = ops.k_wt_level(x, B, H, W, C, 1, taps, K, flip=flip)
    if flip:   # the base conv's input gradient: the depthwise kernel with the flipped taps, no bias
        y0, _, _ = ops.k_dwconv_bwd(x, x, bw, bb, B, H, W, C, K, lib.ACT_NONE, want_w=False)
    else:
        y0 = ops.k_dwconv_fwd(x, bw, bb, B, H, W, C, K, lib.ACT_NONE)
    sub, tag, yb = ops.k_wt_level_base(x, B, H, W, C, taps, bw, bb, K, flip=flip)
    assert torch.equal(sub, sub0), "sub"
    assert torch.equal(tag, tag0), "tag"
    assert torch.equal(yb, y0), "dxb" if flip else "ybase"


class _UnfusedWTConvFn(torch.autograd.Function):
    """ops.WTConvFn's fp32 path before the fusion: the base conv in launches of its own (forward: after the synthesis, which is its addend;
    backward: the depthwise kernel's input gradient)."""

    @staticmethod
    def forward(ctx, x, H, W, K, base_wt, base_bias, *level_wt):
        B, L, C = x.shape
        x2 = x.reshape(B * L, C)
        levels = len(level_wt)
        shapes, subs, tags = [], [], []
        cur, cx, h, w = x2, 1, H, W
        for i in range(levels):
            shapes.append((h, w))
            sub, tag = ops.k_wt_level(cur, B, h, w, C, cx, level_wt[i], K)
            h, w = (h + 1) // 2, (w + 1) // 2
            subs.append(sub)
            tags.append(tag)
            cur, cx = sub, 4
        nxt = ops.k_haar_synthesis(tags, shapes, B, C)
        y = ops.k_dwconv_fwd(x2, base_wt, base_bias, B, H, W, C, K, lib.ACT_NONE, addend=nxt)
        ctx.save_for_backward(x2, base_wt, base_bias, *level_wt, *subs)
        ctx.dims = (B, H, W, C, K, levels, shapes)
        ctx.set_materialize_grads(False)
        return y.view(B, L, C), x

    @staticmethod
    def backward(ctx, dy, dalias):
        B, H, W, C, K, levels, shapes = ctx.dims
        saved = ctx.saved_tensors
        x2, base_wt, base_bias = saved[0], saved[1], saved[2]
        level_wt, subs = saved[3:3 + levels], saved[3 + levels:]
        need_dx = ctx.needs_input_grad[0]
        dy2 = dy.reshape(B * H * W, C).contiguous()
        dxb, dbase, dbb = ops.k_dwconv_bwd(dy2, x2, base_wt, base_bias, B, H, W, C, K, lib.ACT_NONE, want_bias=base_bias is not None, want_dx=need_dx)
        dtags, dsubs = [], []
        cur, cx = dy2, 1
        for i in range(levels):
            hh, ww = shapes[i]
            if need_dx:
                dm, dsub = ops.k_wt_level(cur, B, hh, ww, C, cx, level_wt[i], K, flip=True)
                dsubs.append(dsub)
            else:
                dm = ops.k_haar_dwt(cur, B, hh, ww, C, cx)
            dtags.append(dm)
            cur, cx = dm, 4
        dlw = [None] * levels
        for i in range(levels - 1, -1, -1):
            hh, ww = shapes[i]
            _, dlw[i], _ = ops.k_dwconv_bwd(dtags[i], subs[i], level_wt[i], None, B, (hh + 1) // 2, (ww + 1) // 2, 4 * C, K, lib.ACT_NONE, want_dx=False)
        dx = None
        if need_dx:
            dx = ops.k_haar_synthesis(dsubs, shapes, B, C, y_add=(dxb, dalias.reshape(B * H * W, C) if dalias is not None else None))
        return (dx.view(B, H * W, C) if dx is not None else None, None, None, None, dbase, dbb, *dlw)


def _run_node(fn, x, H, W, K, bw, bb, lws, tap, need_dx, cot, cot_alias):
    x = x.clone().requires_grad_(need_dx)
    bw, bb = bw.clone().requires_grad_(True), bb.clone().requires_grad_(True)
    lws = [t.clone().requires_grad_(True) for t in lws]
    y, xa = fn(x, H, W, K, bw, bb, *lws)
    loss = (y * cot).sum()
    if tap:
        loss = loss + (xa * cot_alias).sum()
    loss.backward()
    torch.cuda.synchronize()
    return y.detach(), x.grad, bw.grad, bb.grad, [t.grad for t in lws]


@pytest.mark.parametrize("B,H,W,C,levels,tap,need_dx", [
    (2, 16, 16, 8, 3, False, True),
    (2, 16, 16, 8, 3, True, True),
    (1, 20, 28, 8, 2, False, True),
    (1, 20, 28, 8, 2, True, True),
    (2, 16, 16, 8, 3, False, False),   # an input that needs no gradient: every input-gradient kernel is skipped
])
def test_wtconv_node_bitwise(B, H, W, C, levels, tap, need_dx):
    K = 5
    tag_ = f"wtn.{H}.{W}"
    x = T(tag_ + ".x", (B, H * W, C))
    bw, bb = T(tag_ + ".bw", (K * K, C), 0.3), T(tag_ + ".bb", (C,), 0.3)
    lws = [T(f"{tag_}.l{i}", (K * K, 4 * C), 0.3) for i in range(levels)]
    cot, cot_alias = T(tag_ + ".c", (B, H * W, C)), T(tag_ + ".ca", (B, H * W, C))
    want = _run_node(_UnfusedWTConvFn.apply, x, H, W, K, bw, bb, lws, tap, need_dx, cot, cot_alias)
    got = _run_node(lambda x_, H_, W_, K_, bw_, bb_, *lw_: ops.wtconv(x_, H_, W_, K_, bw_, bb_, lw_, tap=True), x, H, W, K, bw, bb, lws, tap, need_dx, cot, cot_alias)
    assert torch.equal(got[0], want[0]), "y"
    if need_dx:
        assert torch.equal(got[1], want[1]), "dx"
    else:
        assert got[1] is None and want[1] is None
    assert torch.equal(got[2], want[2]), "d base taps"
    assert torch.equal(got[3], want[3]), "d base bias"
    for i in range(levels):
        assert torch.equal(got[4][i], want[4][i]), f"d level {i} taps"
