"""Gradient accumulation without a GPU: the host-side argument checks of adnm_grad_accum / adnm_grad_accum_final (they return before
any launch), and FlatTrainer(accum_steps=k) on its torch-ops path (fused=False) — the cycle bookkeeping, the accumulator's lifetime and
the arithmetic against the big batch."""
import copy

import pytest
import torch
import torch.nn as nn

from adnm_hip import lib
from adnm_hip.trainer import FlatTrainer


def test_entry_points_reject_bad_arguments_before_any_launch():
    L = lib.load()
    ok = 0x10000   # any 16-byte aligned non-null address: the checks return before the pointers are used
    for args, word in (((None, ok, 8, 1, None), "null"), ((ok, None, 8, 0, None), "null"), ((ok, ok, 0, 0, None), "n <= 0"),
                       ((ok + 4, ok, 8, 0, None), "aligned"), ((ok, ok + 8, 8, 0, None), "aligned"), ((ok, ok, 6, 0, None), "multiple of 4")):
        assert L.adnm_grad_accum(*args) == -1 and word in lib.last_error(), (args, lib.last_error())
    for args, word in (((None, ok, None, 8, 0.5, None), "null"), ((ok, None, ok, 8, 0.5, None), "null"), ((ok, ok, None, -4, 0.5, None), "n <= 0"),
                       ((ok + 4, ok, None, 8, 0.5, None), "aligned"), ((ok, ok + 8, None, 8, 0.5, None), "aligned"),
                       ((ok, ok, ok + 2, 8, 0.5, None), "aligned"), ((ok, ok, ok, 6, 0.5, None), "multiple of 4")):
        assert L.adnm_grad_accum_final(*args) == -1 and word in lib.last_error(), (args, lib.last_error())
    assert L.adnm_abi_version() == 11


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.a, self.b = nn.Linear(8, 16), nn.Linear(16, 4)
        self.dead = nn.Linear(4, 4)   # never used: stays out of the flat buffers

    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))


def _trainer(model, **kw):
    return FlatTrainer(model, lambda o, t: (o - t).pow(2).mean(), lr=1e-2, eps=1e-9, weight_decay=1e-2, max_norm=0.5, use_graph=False, fused=False, **kw)


def test_accum_steps_one_allocates_nothing_and_bad_values_raise():
    tr = _trainer(Net())
    tr.step(torch.randn(4, 8), torch.randn(4, 4))
    assert tr.accum_steps == 1 and tr.micro_step == 0 and tr.acc is None and tr._steps == 1
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            _trainer(Net(), accum_steps=bad)
        with pytest.raises(ValueError):
            tr.accum_steps = bad
    tr.close()


def test_cycle_bookkeeping_and_accumulator_lifetime():
    torch.manual_seed(1)
    tr = _trainer(Net(), accum_steps=3)
    x, t = torch.randn(4, 8), torch.randn(4, 4)
    tr.step(x, t)
    assert tr.acc is not None and tr.acc.shape == tr.flat_g.shape and tr.micro_step == 1 and tr._steps == 0
    p0, m0 = tr.flat_p.clone(), tr.exp_avg.clone()
    with pytest.raises(RuntimeError, match="mid-cycle"):
        tr.accum_steps = 2
    tr.step(x, t)
    assert tr.micro_step == 2 and tr._steps == 0 and torch.equal(tr.flat_p, p0) and torch.equal(tr.exp_avg, m0)
    tr.step(x, t)
    assert tr.micro_step == 0 and tr._steps == 1 and not torch.equal(tr.flat_p, p0)
    tr.accum_steps = 1          # between cycles: allowed; the accumulator goes
    assert tr.acc is None
    tr.step(x, t)
    assert tr._steps == 2 and tr.acc is None
    tr.accum_steps = 2
    tr.step(x, t)
    assert tr.acc is not None and tr.micro_step == 1
    tr.close()
    assert tr.acc is None and tr.micro_step == 0


def test_micro_batches_equal_the_big_batch_on_the_torch_path():
    """k = 4 micro-batches of 2 against torch.optim.AdamW on the batch of 8 (mean loss), 3 optimiser steps; the bar is the one
    tests/test_ddp_gloo.py uses for the same comparison across ranks."""
    k = 4
    torch.manual_seed(2)
    mine = Net()
    ref = copy.deepcopy(mine)
    tr = _trainer(mine, accum_steps=k)
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-2, eps=1e-9, weight_decay=1e-2)
    for _ in range(3):
        x, t = torch.randn(2 * k, 8), torch.randn(2 * k, 4)
        losses = [float(tr.step(x[2 * i:2 * i + 2], t[2 * i:2 * i + 2]).detach()) for i in range(k)]
        loss_ref = (ref(x) - t).pow(2).mean()
        loss_ref.backward()
        norm_ref = torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.5)
        opt.step()
        opt.zero_grad(set_to_none=True)
        assert abs(sum(losses) / k - float(loss_ref.detach())) <= 1e-5 * abs(float(loss_ref.detach()))
        assert abs(float(tr.grad_norm()) - float(norm_ref)) <= 1e-4 * float(norm_ref)
    for (name, a), (_, b) in zip(mine.named_parameters(), ref.named_parameters()):
        assert torch.allclose(a, b, atol=2e-6, rtol=1e-5), name
    tr.close()
