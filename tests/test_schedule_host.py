"""adnm_hip.schedule.ReferenceSchedule on the host: the learning rate against torch's own LinearLR + CosineAnnealingLR + SequentialLR
(train_untils.py:44-46), the clip threshold against the formula of train.py:122-130 for both parameter sets (train.py:78-94), and
apply() against a stub trainer."""
import pytest
import torch

from adnm_hip.schedule import ReferenceSchedule

# (input_frames, frame_interval) on either side of frame_interval < 120 / input_frames, and the parameter set each must select
RECIPES = [((5, 6), dict(save_epoch=34, norm_ratio=1.75, norm_max=0.025, norm_initial=0.175, excursion=1)),
           ((5, 30), dict(save_epoch=20, norm_ratio=3.0, norm_max=0.035, norm_initial=0.065, excursion=0))]


def test_lr_equals_torchs_sequential_schedule():
    """e = 0 .. 39: what the optimiser holds after e scheduler steps.  Both sides are Python floats (fp64); 1e-12 relative leaves room
    for torch's recursive form of the cosine (one rounding per epoch) against the closed form."""
    p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    opt = torch.optim.AdamW([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2)
    warm = torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.01, total_iters=3)
    cos = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=50, eta_min=5e-7)
    sched = torch.optim.lr_scheduler.SequentialLR(opt, [warm, cos], [3])
    mine = ReferenceSchedule(5, 6)
    assert mine.epochs == 40
    for e in range(40):
        want = opt.param_groups[0]["lr"]
        got = mine.lr(e)
        assert abs(got - want) <= 1e-12 * abs(want), (e, got, want)
        opt.step()
        sched.step()
    assert mine.lr(0) == 1e-3 * 0.01 and mine.lr(3) == 1e-3


@pytest.mark.parametrize("args,par", RECIPES)
def test_max_norm_follows_the_reference_formula(args, par):
    s = ReferenceSchedule(*args)
    assert s.short_interval == (args[1] < 120 / args[0])
    for k, v in par.items():
        assert getattr(s, k) == v, k
    w, prev = s.warmup_epochs, 0.0123
    ramp_end = par["save_epoch"] - w + par["excursion"]
    assert s.ramp_end == ramp_end
    # train.py counts epochs from 1: e1 = epoch + 1.  norm_max through e1 = warmup + 1, whatever the previous epoch's norm was
    for e1 in range(1, w + 2):
        assert s.max_norm(e1 - 1, prev) == par["norm_max"] and s.max_norm(e1 - 1, None) == par["norm_max"]
    # the ramp: the reference's own expression, term for term
    for e1 in range(w + 2, ramp_end + 1):
        alpha = par["norm_initial"] + (1 - par["norm_initial"]) * (e1 - w) / ramp_end
        assert s.max_norm(e1 - 1, prev) == alpha * par["norm_ratio"] * prev, e1
    # at its end the factor is the one the formula implies — below 1: the threshold steps up one epoch later, by exactly that factor
    last = par["norm_initial"] + (1 - par["norm_initial"]) * (ramp_end - w) / ramp_end
    assert last < 1.0
    assert s.max_norm(ramp_end - 1, prev) == last * par["norm_ratio"] * prev
    assert s.max_norm(ramp_end, prev) == par["norm_ratio"] * prev
    # monotone inside the ramp
    ramp = [s.max_norm(e1 - 1, prev) for e1 in range(w + 2, ramp_end + 2)]
    assert all(a < b for a, b in zip(ramp, ramp[1:]))
    for e1 in range(ramp_end + 1, s.epochs + 1):
        assert s.max_norm(e1 - 1, prev) == par["norm_ratio"] * prev
    with pytest.raises(ValueError):
        s.max_norm(w + 1, None)


def test_pinned_values():
    """figures worked out by hand from train.py:78-94, 122-130 and train_untils.py:44-46, not from the code under test.
    Epoch 10 (train.py's 11th), previous mean norm 0.02:
      short interval: ramp_end = 34 - 3 + 1 = 32, alpha = 0.175 + 0.825 * 8 / 32 = 0.38125,    0.38125 * 1.75 * 0.02 = 0.01334375
      long interval:  ramp_end = 20 - 3 + 0 = 17, alpha = 0.065 + 0.935 * 8 / 17 = 0.505,      0.505 * 3 * 0.02 = 0.0303
    learning rate: 1e-5 at epoch 0; 0.01 + 0.99 / 3 = 0.34 of 1e-3 at epoch 1; 1e-3 at epoch 3; epoch 28 is the cosine's midpoint
    (cos(pi / 2) = 0): (1e-3 + 5e-7) / 2 = 5.0025e-4"""
    short, long_ = ReferenceSchedule(5, 6), ReferenceSchedule(5, 60)
    assert short.max_norm(10, 0.02) == pytest.approx(0.01334375, rel=1e-12)
    assert long_.max_norm(10, 0.02) == pytest.approx(0.0303, rel=1e-12)
    assert short.max_norm(32, 0.02) == pytest.approx(0.035, rel=1e-12) and long_.max_norm(17, 0.02) == pytest.approx(0.06, rel=1e-12)
    assert short.lr(0) == pytest.approx(1e-5, rel=1e-12) and short.lr(1) == pytest.approx(3.4e-4, rel=1e-12)
    assert short.lr(3) == pytest.approx(1e-3, rel=1e-12) and short.lr(28) == pytest.approx(5.0025e-4, rel=1e-12)


def test_apply_sets_exactly_two_attributes():
    class Stub:
        pass
    t = Stub()
    s = ReferenceSchedule(5, 6)
    lr, mn = s.apply(t, 0, None)
    assert vars(t) == {"lr": s.lr(0), "max_norm": 0.025} and (lr, mn) == (t.lr, t.max_norm)
    s.apply(t, 10, {"norm_mean": 0.02, "steps": 7})
    assert vars(t) == {"lr": s.lr(10), "max_norm": s.max_norm(10, 0.02)}
    assert t.max_norm != 0.025
