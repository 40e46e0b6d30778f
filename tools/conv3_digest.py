#!/usr/bin/env python3
"""SHA-256 of what ops.conv3 computes — y, dx, dw, db of one forward + backward with a contiguous cotangent — on every shape of
test_conv3 and test_conv3_bf16_mfma in f32 and bf16, and on test_conv3_fp8_mfma's shape in fp8 with its explicit scales.  The op's Python
surface is stable, so two checkouts (each with its own built library) can be compared line by line: a kernel refactor that keeps the MFMA
sequence and the summation order prints the same digests.   python tools/conv3_digest.py"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "adnm-unet_amd"))
import torch
from adnm_hip import lib, ops, recipe

DEV = "cuda"
G, NO = lib.ACT_GELU, lib.ACT_NONE
# (B, H, W, K, N, act, bias, channels-last weight)
SHAPES = [(2, 16, 16, 5, 32, G, False, False), (4, 128, 128, 64, 32, G, True, True), (2, 8, 8, 256, 64, G, True, True),
          (1, 4, 4, 64, 128, NO, True, False), (2, 12, 12, 16, 24, G, True, False), (1, 64, 64, 20, 20, NO, False, True),
          (2, 7, 9, 8, 12, G, True, False), (1, 32, 32, 32, 200, NO, True, True),                                    # test_conv3
          (2, 16, 16, 32, 64, NO, True, False), (1, 32, 32, 5, 32, G, True, False), (2, 8, 8, 20, 20, NO, True, False),
          (1, 16, 16, 128, 32, G, True, False), (4, 4, 4, 256, 64, NO, True, False), (1, 8, 8, 144, 48, G, True, False),
          (2, 4, 4, 512, 128, G, True, False), (1, 24, 40, 72, 16, NO, True, False)]                                 # test_conv3_bf16_mfma


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest() if t is not None else "-" * 64


def run(tag, B, H, W, K, N, act, bias, cl, scales=None):
    name = f"{B}.{H}.{W}.{K}.{N}"
    x, w, cot = recipe.tensor("dg.x" + name, (B, H * W, K)), recipe.tensor("dg.w" + name, (N, K, 3, 3), 0.2), recipe.tensor("dg.c" + name, (B, H * W, N))
    xg = x.to(DEV).requires_grad_(True)
    wg = w.to(DEV)
    if cl:
        wg = wg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    wg = wg.detach().requires_grad_(True)
    bg = recipe.tensor("dg.b" + name, (N,)).to(DEV).requires_grad_(True) if bias else None
    if scales:   # (fmax of e4m3, fmax of e5m2): one binade of headroom under each, as test_conv3_fp8_mfma sets them
        sx, sw, sc = scales[0] / (2.0 * float(x.abs().max())), scales[0] / (2.0 * float(w.abs().max())), scales[1] / (2.0 * float(cot.abs().max()))
        ops.QUANT.set(xg.device, wg.data_ptr(), "conv3_fwd", sx, sw)
        ops.QUANT.set(xg.device, wg.data_ptr(), "conv3_dgrad", sc, sw)
    y = ops.conv3(xg, wg, bg, H, W, act)
    y.backward(cot.to(DEV))
    torch.cuda.synchronize()
    dw = wg.grad.permute(0, 2, 3, 1) if cl else wg.grad
    print(f"{tag:4s} {B}x{H}x{W} {K:3d}->{N:<3d} act {act} bias {int(bias)} cl {int(cl)}  y {sha(y)}  dx {sha(xg.grad)}  dw {sha(dw)}  db {sha(bg.grad if bias else None)}",
          flush=True)


for prec in ("f32", "bf16"):
    ops.set_mfma_precision(prec)
    for s in SHAPES:
        run(prec, *s)
ops.QUANT.reset()
ops.set_mfma_precision("fp8")
ops.QUANT.max_rows = 1 << 30
run("fp8", 2, 16, 16, 32, 64, NO, True, False, scales=(448.0, 57344.0))
ops.set_mfma_precision("f32")
