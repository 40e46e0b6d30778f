"""ReferenceSelection (adnm_hip.schedule): the best-checkpoint gate and the early stop of train.py:169-183, 205 against decision
sequences written out by hand, for both recipes; host only."""
import math

import pytest

from adnm_hip.schedule import ReferenceSchedule, ReferenceSelection


def _short():
    return ReferenceSchedule(input_frames=5, frame_interval=6)      # 6 < 120 / 5: save_epoch 34, early_stop 3


def _long():
    return ReferenceSchedule(input_frames=5, frame_interval=60)     # save_epoch 20, early_stop 5


def _run(sel, first_epoch, losses):
    return [(d["save"], d["stop"], d["best"], d["bad_epochs"]) for d in (sel.update(first_epoch + i, v) for i, v in enumerate(losses))]


def test_recipes():
    s, l = ReferenceSelection(_short()), ReferenceSelection(_long())
    assert (s.save_epoch, s.early_stop, s.best, s.bad_epochs) == (34, 3, 10000.0, 0)
    assert (l.save_epoch, l.early_stop, l.best, l.bad_epochs) == (20, 5, 10000.0, 0)


@pytest.mark.parametrize("make,save_epoch", [(_short, 34), (_long, 20)])
def test_nothing_happens_up_to_save_epoch_and_the_first_eligible_epoch_saves(make, save_epoch):
    sel = ReferenceSelection(make())
    for epoch in range(save_epoch):     # e1 = 1 .. save_epoch: however good (or bad, or broken) the loss
        d = sel.update(epoch, (1e-3, 5e4, float("nan"))[epoch % 3])
        assert d == {"save": False, "stop": False, "best": 10000.0, "bad_epochs": 0}, (epoch, d)
    d = sel.update(save_epoch, 9999.0)   # e1 = save_epoch + 1: any loss below 10000 is the best so far
    assert d == {"save": True, "stop": False, "best": 9999.0, "bad_epochs": 0}


def test_short_recipe_sequence_by_hand():
    sel = ReferenceSelection(_short())
    got = _run(sel, 34, [5.0, 5.0, 4.0, float("nan"), 4.5, 3.9, 3.9, 4.0, float("inf"), 1.0])
    assert got == [(True, False, 5.0, 0),     # first eligible epoch
                   (False, False, 5.0, 1),    # an equal loss is not better
                   (True, False, 4.0, 0),     # improvement: the counter goes back to 0
                   (False, False, 4.0, 1),    # NaN is not better
                   (False, False, 4.0, 2),
                   (True, False, 3.9, 0),     # saved at 2 bad epochs: no stop
                   (False, False, 3.9, 1),
                   (False, False, 3.9, 2),
                   (False, True, 3.9, 3),     # the 3rd consecutive bad epoch, exactly
                   (True, False, 1.0, 0)]     # (the caller has left the loop; the rule itself goes on)


def test_long_recipe_stops_at_the_fifth_bad_epoch():
    sel = ReferenceSelection(_long())
    got = _run(sel, 19, [0.1, 7.0, 8.0, 8.0, 9.0, 7.5, 6.0, 6.5, 6.5, float("nan"), 6.0, 7.0])
    assert got == [(False, False, 10000.0, 0),   # e1 = 20 = save_epoch: not eligible yet, the excellent loss is ignored
                   (True, False, 7.0, 0),
                   (False, False, 7.0, 1), (False, False, 7.0, 2), (False, False, 7.0, 3), (False, False, 7.0, 4),
                   (True, False, 6.0, 0),       # 4 bad epochs, then an improvement
                   (False, False, 6.0, 1), (False, False, 6.0, 2), (False, False, 6.0, 3), (False, False, 6.0, 4),
                   (False, True, 6.0, 5)]


def test_a_nan_in_the_first_eligible_epoch_is_bad_and_best_stays():
    sel = ReferenceSelection(_short())
    d = sel.update(34, float("nan"))
    assert d["save"] is False and d["bad_epochs"] == 1 and d["best"] == 10000.0 and not math.isnan(d["best"])


@pytest.mark.parametrize("make,first", [(_short, 34), (_long, 20)])
def test_state_dict_round_trip_mid_sequence(make, first):
    losses = [5.0, 6.0, 4.0, 4.0, float("nan"), 4.1, 4.2, 4.3, 3.0]
    whole = _run(ReferenceSelection(make()), first, losses)
    for cut in range(1, len(losses)):
        a = ReferenceSelection(make())
        head = _run(a, first, losses[:cut])
        sd = a.state_dict()
        assert all(type(v) in (int, float) for v in sd.values()), sd     # plain scalars: goes into schedule_stats as it is
        b = ReferenceSelection(make())
        b.load_state_dict(dict(sd))
        assert head + _run(b, first + cut, losses[cut:]) == whole, cut


def test_a_state_of_the_other_recipe_is_refused():
    sd = ReferenceSelection(_short()).state_dict()
    with pytest.raises(ValueError, match="save_epoch"):
        ReferenceSelection(_long()).load_state_dict(sd)


def test_selection_state_travels_in_a_training_state_file(tmp_path):
    """checkpoint.save_training_state's schedule_stats takes the dict unchanged (torch.save of Python scalars)"""
    import torch
    sel = ReferenceSelection(_short())
    _run(sel, 34, [5.0, 6.0])
    path = str(tmp_path / "sel.pth")
    torch.save({"schedule_stats": {"selection": sel.state_dict()}}, path)
    back = ReferenceSelection(_short())
    back.load_state_dict(torch.load(path)["schedule_stats"]["selection"])
    assert back.state_dict() == sel.state_dict() == {"best": 5.0, "bad_epochs": 1, "save_epoch": 34, "early_stop": 3}


_fixture = {}


def _fixture_block():
    """-> (the reference's fixture, thresholds, hw, SSIM area, the (T, 4 * nthr + 3) table of a block) built from the oracle's per-frame
    counts of the reference's own fixture, once"""
    if not _fixture:
        import numpy as np
        import adnm_oracle as O
        from util import load_npz
        z = load_npz("evaluator_b3_t5")
        thr, scale = [20, 30, 35, 40], float(z["value_scale"])
        counts, mae, mse = O.evaluator_counts(z["truth"], z["pred"], scale, thr)
        ssim = O.evaluator_ssim(z["truth"], z["pred"], scale)
        hw, area = 48 * 48, 38 * 38
        tab = np.zeros((5, 4 * 4 + 3))
        for k, t in enumerate(thr):
            tab[:, 4 * k:4 * k + 4] = counts[t].double().sum(0).numpy()     # (B, T, [TP, FN, FP, TN]) summed over the samples
        tab[:, 16], tab[:, 17], tab[:, 18] = (mae.double() * hw).sum(0).numpy(), (mse.double() * hw).sum(0).numpy(), (ssim.double() * area).sum(0).numpy()
        tab.setflags(write=False)
        _fixture["v"] = (z, thr, hw, area, tab)
    return _fixture["v"]


def test_aggregate_of_a_block_built_by_the_oracle_matches_the_reference_fixture():
    """Validator.done()'s host half: per-frame-index sums (what the device block holds) are enough for every score of
    SimplifiedEvaluator.done — the block is built here from the oracle's per-frame counts of the reference's own fixture."""
    import numpy as np
    from adnm_hip.validate import aggregate
    z, thr, hw, area, tab = _fixture_block()
    res = aggregate(np.concatenate([[1.25, 2, 3, 0], tab.ravel()]), thr, 5, hw, area)
    for t in thr:
        m = res["threshold_metrics"][t]
        for k in ("TP", "TN", "FP", "FN"):
            assert m[k] == float(z[f"{k}.{t}"]), (t, k)
        for k in ("CSI", "POD", "HSS"):
            assert abs(m[k] - float(z[f"{k}.{t}"])) <= 1e-9, (t, k)
    assert abs(res["FAR"] - float(z["FAR"])) <= 1e-9 and abs(res["SSIM"] - float(z["SSIM"])) <= 1e-9
    assert abs(res["RMSE"] - float(z["RMSE"])) <= 1e-5 * float(z["RMSE"]) and abs(res["MSE"] - float(z["mse"].mean())) <= 1e-5 * float(z["mse"].mean())
    assert abs(res["MAE"] - float(z["mae"].mean())) <= 1e-5 * float(z["mae"].mean())
    assert (res["loss_sum"], res["loss_mean"], res["batches"], res["samples"], res["nonfinite"]) == (1.25, 0.625, 2, 3, 0)
    assert aggregate(np.concatenate([[0, 0, 3, 0], tab.ravel()]), thr, 5, hw, None)["SSIM"] is None


def test_contingency_metrics_is_the_one_statement_both_evaluators_use():
    """evaluator.contingency_metrics on the counts of the reference's fixture gives what aggregate() gives on the block above, value for
    value (NaN with NaN), and GpuEvaluator.done() goes through it too: its tables are filled by hand with CPU tensors (done() only
    reads them)."""
    import numpy as np
    import torch
    from adnm_hip import evaluator
    from adnm_hip.validate import aggregate
    z, thr, hw, area, tab = _fixture_block()
    same = lambda a, b: a == b or (np.isnan(a) and np.isnan(b))
    sums = tab[:, :16].sum(axis=0)
    metrics, far = evaluator.contingency_metrics(sums, thr)
    res = aggregate(np.concatenate([[1.25, 2, 3, 0], tab.ravel()]), thr, 5, hw, area)
    assert list(metrics) == list(res["threshold_metrics"]) == thr and len(far) == 4
    for t in thr:
        assert metrics[t].keys() == res["threshold_metrics"][t].keys()
        assert all(same(metrics[t][k], res["threshold_metrics"][t][k]) for k in metrics[t]), t
        for k in ("TP", "TN", "FP", "FN"):
            assert metrics[t][k] == float(z[f"{k}.{t}"]), (t, k)
        for k in ("CSI", "POD", "HSS"):
            assert abs(metrics[t][k] - float(z[f"{k}.{t}"])) <= 1e-9, (t, k)
    assert same(float(np.mean(far)), res["FAR"]) and abs(res["FAR"] - float(z["FAR"])) <= 1e-9
    # GpuEvaluator.done(): one (B, T, 4 * nthr + 2) fp32 table per evaluate() call; the same counts spread over two calls
    ev = evaluator.GpuEvaluator(5, float(z["value_scale"]), thr)
    a, b = torch.zeros(2, 5, 18), torch.zeros(1, 5, 18)
    a[1, 2, :16], b[0, 4, :16] = torch.from_numpy(sums - 7.0).float(), 7.0
    a[..., 17], b[..., 17] = 3.0, 5.0
    assert torch.equal(a[1, 2, :16].double() + 7.0, torch.from_numpy(sums)), "the fixture's counts are not exact in fp32: nothing is tested"
    ev._tables, ev._ssim = [(a, hw), (b, hw)], []
    done = ev.done()
    assert list(done["threshold_metrics"]) == thr
    for t in thr:
        assert all(same(done["threshold_metrics"][t][k], metrics[t][k]) for k in metrics[t]), t
    assert same(done["FAR"], res["FAR"]) and done["SSIM"] is None
    # a threshold nothing crosses: 0 / 0 without a warning, and a non-integer key kept as it is
    m0, f0 = evaluator.contingency_metrics(np.array([0.0, 0.0, 0.0, 10.0]), [2.5])
    assert list(m0) == [2.5] and np.isnan(m0[2.5]["CSI"]) and np.isnan(m0[2.5]["POD"]) and np.isnan(f0[0]) and m0[2.5]["TN"] == 10.0
    calls = []
    real, evaluator.contingency_metrics = evaluator.contingency_metrics, lambda s, th: calls.append(1) or real(s, th)
    try:
        ev.done()
    finally:
        evaluator.contingency_metrics = real
    assert calls == [1], "GpuEvaluator.done() does not go through contingency_metrics"
