"""Gradient accumulation on the GPU (FlatTrainer(accum_steps=k), adnm_grad_accum / adnm_grad_accum_final): train.py:136-145 with
loss.backward() repeated k times before optimizer.step().  The kernels against torch bit for bit; the trainer against an independent
torch loop (autograd's own accumulation, clip_grad_norm_, torch.optim.AdamW), against itself without accumulation (bitwise), and
against the big batch the micro-batches add up to."""
import copy

import pytest
import torch

from adnm_hip import lib, ops, recipe
from adnm_hip.trainer import FlatTrainer
from util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the kernels run <= 2048 workgroups of 256 lanes, one float4 per lane and trip.  Two full grid-stride trips of EVERY lane need
# 2 * 2048 * 256 = 1 048 576 quads = 4 194 304 elements; one quad more (+4) starts a third trip on lane 0 alone and makes n % 8 == 4
GRID_LANES = 2048 * 256
N_TWO_TRIPS = 2 * GRID_LANES * 4 + 4


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _vals(name, n):
    return recipe.tensor(name, (n,)).to(DEV)


@pytest.mark.parametrize("n", [4, 1020, N_TWO_TRIPS])
def test_accum_kernels_match_torch_exactly(n):
    assert n % 4 == 0 and (n < 8 or n % 8 == 4) and (n < GRID_LANES or n // 4 > 2 * GRID_LANES)
    g1, g2, g3 = _vals("acc.g1", n), _vals("acc.g2", n), _vals("acc.g3", n)
    acc = torch.full((n,), float("nan"), device=DEV)
    lib.call("adnm_grad_accum", acc.data_ptr(), g1.data_ptr(), n, 1, _stream())
    assert torch.equal(acc, g1), "first != 0 must overwrite the accumulator without reading it (NaN pre-fill)"
    lib.call("adnm_grad_accum", acc.data_ptr(), g2.data_ptr(), n, 0, _stream())
    want = g1 + g2
    assert torch.equal(acc, want)
    for scale in (1.0 / 3.0, 1.0 / 8.0):
        g = g3.clone()
        sentinel = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
        wire = sentinel.clone()
        lib.call("adnm_grad_accum_final", acc.data_ptr(), g.data_ptr(), None, n, scale, _stream())
        ref = (want + g3) * scale
        assert torch.equal(g, ref), f"scale {scale}: g != (acc + g) * scale"
        assert torch.equal(wire, sentinel), "wire = NULL must not touch any wire buffer"
        assert torch.equal(acc, want), "the final pass must not write the accumulator"
        g = g3.clone()
        lib.call("adnm_grad_accum_final", acc.data_ptr(), g.data_ptr(), wire.data_ptr(), n, scale, _stream())
        assert torch.equal(g, ref)
        assert torch.equal(wire, ref.to(torch.bfloat16)), f"scale {scale}: wire != bf16(g)"


def test_accum_kernels_on_a_sub_range_leave_the_rest_alone():
    total, lo, hi = 4096, 1000, 1000 + 2052
    assert lo % 8 == 0 and lo > 0 and (hi - lo) % 8 == 4 and hi < total
    n = hi - lo
    g0, a0 = _vals("sub.g", total), _vals("sub.a", total)
    g, acc = g0.clone(), a0.clone()
    wire0 = torch.full((total,), 7.0, dtype=torch.bfloat16, device=DEV)
    wire = wire0.clone()

    def outside_untouched(t, t0):
        return torch.equal(t[:lo], t0[:lo]) and torch.equal(t[hi:], t0[hi:])
    lib.call("adnm_grad_accum", acc[lo:hi].data_ptr(), g[lo:hi].data_ptr(), n, 0, _stream())
    assert torch.equal(acc[lo:hi], a0[lo:hi] + g0[lo:hi]) and outside_untouched(acc, a0) and torch.equal(g, g0)
    lib.call("adnm_grad_accum", acc[lo:hi].data_ptr(), g[lo:hi].data_ptr(), n, 1, _stream())
    assert torch.equal(acc[lo:hi], g0[lo:hi]) and outside_untouched(acc, a0) and torch.equal(g, g0)
    acc = a0.clone()
    lib.call("adnm_grad_accum_final", acc[lo:hi].data_ptr(), g[lo:hi].data_ptr(), wire[lo:hi].data_ptr(), n, 1.0 / 3.0, _stream())
    ref = (a0[lo:hi] + g0[lo:hi]) * (1.0 / 3.0)
    assert torch.equal(g[lo:hi], ref) and outside_untouched(g, g0) and torch.equal(acc, a0)
    assert torch.equal(wire[lo:hi], ref.to(torch.bfloat16)) and outside_untouched(wire, wire0)


def small_model():
    from models.ADNMUNet import create_block
    torch.manual_seed(0)
    m = create_block(32, 16, headdim=4, norm_epsilon=1e-6)
    recipe.fill_parameters(m)
    return m.to(DEV)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("max_norm", [0.0, 0.05])
def test_three_micro_batches_match_torch_accumulation(use_graph, max_norm):
    """k = 3 (1/3 is not a power of two), three DIFFERENT micro-batches per cycle, 3 cycles, against a deep copy driven by torch alone:
    (loss_i / 3).backward() three times (autograd adds into p.grad), clip_grad_norm_, torch.optim.AdamW.step.  The bars are those of
    test_trainer_gpu.test_fused_step_matches_torch."""
    k = 3
    ref = small_model()
    mine = copy.deepcopy(ref)
    xs = [recipe.tensor(f"acc3.x{i}", (2, 64, 32)).to(DEV) for i in range(3 * k)]
    ts = [recipe.tensor(f"acc3.t{i}", (2, 64, 16)).to(DEV) for i in range(3 * k)]
    loss_fn = lambda o, t: ((o - t) ** 2).mean()
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2)
    tr = FlatTrainer(mine, loss_fn, lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=max_norm, use_graph=use_graph, accum_steps=k)
    try:
        for cycle in range(3):
            for i in range(k):
                x, t = xs[cycle * k + i], ts[cycle * k + i]
                loss_ref = loss_fn(ref(x), t)
                (loss_ref / k).backward()
                assert tr.micro_step == i
                loss = tr.step(x, t)
                assert abs(float(loss) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref)) + 1e-7
            assert tr.micro_step == 0 and tr._steps == cycle + 1 and float(tr.state[0]) == cycle + 1
            if max_norm > 0:
                norm_ref = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
            else:
                norm_ref = torch.stack([p.grad.norm() for p in ref.parameters() if p.grad is not None]).norm()
            opt.step()
            opt.zero_grad(set_to_none=True)
            assert abs(float(tr.grad_norm()) - float(norm_ref)) <= 1e-4 * float(norm_ref)
        for (name, a), (_, b) in zip(mine.named_parameters(), ref.named_parameters()):
            assert_close(a, b, 2e-5, name, atol=1e-6)
    finally:
        tr.close()


def _unet64():
    from models.ADNMUNet import create_ADNMUNet
    model = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(model)
    return model.to(DEV).train()


def _unet_trainer(model, **kw):
    from models.loss import enRainfallLoss
    return FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025, **kw)


@pytest.mark.parametrize("use_graph,overlap", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("prec", ["f32", "bf16", "fp8"])
def test_same_micro_batch_twice_is_bitwise_the_plain_step(prec, use_graph, overlap):
    """k = 2 on the SAME micro-batch: (g + g) * 0.5 == g exactly in fp32, so after every cycle flat_g — and after 3 optimiser steps
    flat_p and exp_avg — must be bit for bit what a plain trainer stepping on that batch holds.  Cycles 2 and 3 check that the first
    micro-step of a cycle restarts the accumulator (a leftover sum would double the gradient).  fp8: the table update runs once per
    optimiser step, and the maxima collected over two identical micro-batches are those of one."""
    frames = recipe.radar_batch(1, 25, 64, name="accum2").to(DEV)
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    runs = []
    ops.set_mfma_precision(prec)
    try:
        for k in (1, 2):
            ops.QUANT.reset()
            tr = _unet_trainer(_unet64(), use_graph=use_graph, overlap=overlap, accum_steps=k)
            try:
                gs = []
                for _ in range(3):
                    for _ in range(k):
                        tr.step(x, tgt)
                    gs.append(tr.flat_g.clone())
                torch.cuda.synchronize()
                assert tr.staged == overlap and (tr.graph is not None) == use_graph and (tr.acc is not None) == (k > 1)
                assert tr.shadow_mode == {"f32": 0, "bf16": 1, "fp8": 2}[prec] and tr._steps == 3
                if prec == "bf16":
                    assert torch.equal(tr.shadow, tr.flat_p.to(torch.bfloat16)), "the shadow is bf16(p) after every optimiser step"
                runs.append((gs, tr.flat_p.clone(), tr.exp_avg.clone(), tr.shadow.clone() if tr.shadow is not None else None))
            finally:
                tr.close()
            del tr
    finally:
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()
    plain, accum = runs
    for c in range(3):
        assert torch.equal(plain[0][c], accum[0][c]), f"flat_g differs after cycle {c + 1}"
    assert torch.equal(plain[1], accum[1]), "flat_p differs after 3 optimiser steps"
    assert torch.equal(plain[2], accum[2]), "exp_avg differs after 3 optimiser steps"
    if plain[3] is not None:
        assert torch.equal(plain[3], accum[3]), "the weight shadow differs after 3 optimiser steps"


def test_two_micro_batches_equal_their_concatenation():
    """f32, 64x64 model: two different B = 1 micro-batches with k = 2 against ONE plain step on their B = 2 concatenation — the same
    gradient up to fp32 summation order (no batch-coupled statistics anywhere in the model, the loss is a mean over all elements).
    flat_g after the first optimiser step is held to the project's fp32 gradient bar, 1e-3 relative L2 (README), and to the same
    figure for max-abs over max; the two micro-losses average to the big-batch loss within 1e-5.  The measured figures are printed."""
    frames = recipe.radar_batch(2, 25, 64, name="accumcat").to(DEV)
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    big = _unet_trainer(_unet64(), use_graph=False)
    try:
        loss_big = float(big.step(x, tgt))
        g_big = big.flat_g.double()
    finally:
        big.close()
    tr = _unet_trainer(_unet64(), use_graph=False, accum_steps=2)
    try:
        l0 = float(tr.step(x[0:1].contiguous(), tgt[0:1].contiguous()))
        l1 = float(tr.step(x[1:2].contiguous(), tgt[1:2].contiguous()))
        g = tr.flat_g.double()
    finally:
        tr.close()
    rel = float((g - g_big).norm() / g_big.norm())
    mx = float((g - g_big).abs().max() / g_big.abs().max())
    dl = abs(0.5 * (l0 + l1) - loss_big) / abs(loss_big)
    print(f"accum equivalence (2 x B=1 vs B=2, 64x64, f32): flat_g rel-L2 {rel:.3e}, max-abs / max {mx:.3e}, mean micro-loss vs big-batch loss {dl:.3e}")
    assert dl <= 1e-5, (l0, l1, loss_big)
    assert rel <= 1e-3, rel
    assert mx <= 1e-3, mx


def test_accumulator_lifetime_and_frozen_state_inside_a_cycle():
    """accum_steps == 1 allocates nothing; inside a cycle neither the parameters nor the moments, the device step counter or (fp8) the
    quantisation table's scales move, and accum_steps cannot be assigned; between cycles it can; close() gives the accumulator back."""
    frames = recipe.radar_batch(1, 25, 64, name="accumguard").to(DEV)
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    ops.set_mfma_precision("fp8")
    try:
        ops.QUANT.reset()
        plain = _unet_trainer(_unet64(), use_graph=False)
        try:
            plain.step(x, tgt)
            assert plain.acc is None and plain.accum_steps == 1 and plain.micro_step == 0
        finally:
            plain.close()
        ops.QUANT.reset()
        k = 3
        tr = _unet_trainer(_unet64(), use_graph=True, accum_steps=k)
        try:
            tr.prepare(x, tgt)
            assert tr.acc is not None and tr.acc.shape == tr.flat_g.shape and tr.acc.dtype == torch.float32 and tr.fp8
            nrec = len(ops.QUANT.dump(x.device))
            assert nrec > 0

            def frozen():
                return [t.clone() for t in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.state[0:1], tr.shadow, ops.QUANT.table(x.device)[:nrec, 0:2])]
            for cycle in range(2):
                before = frozen()
                for i in range(k - 1):
                    tr.step(x, tgt)
                    assert tr.micro_step == i + 1 and tr._steps == cycle
                    for a, b in zip(before, frozen()):
                        assert torch.equal(a, b), "a micro-step inside a cycle moved optimiser state"
                    with pytest.raises(RuntimeError, match="mid-cycle"):
                        tr.accum_steps = 2
                tr.step(x, tgt)
                assert tr.micro_step == 0 and tr._steps == cycle + 1 and float(tr.state[0]) == cycle + 1
                assert not torch.equal(before[0], tr.flat_p), "the last micro-step ran no optimiser pass"
            tr.accum_steps = 2   # between cycles: allowed
            tr.step(x, tgt)
            tr.step(x, tgt)
            assert tr._steps == 3 and tr.micro_step == 0
            tr.accum_steps = 1
            assert tr.acc is None
            tr.step(x, tgt)
            assert tr._steps == 4 and tr.acc is None
            tr.accum_steps = 2
            tr.step(x, tgt)
            assert tr.acc is not None
        finally:
            tr.close()
        assert tr.acc is None and tr.micro_step == 0
    finally:
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()
