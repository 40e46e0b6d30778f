"""The validation epoch on the device (csrc/dataio.hip: adnm_valid_accum / adnm_valid_ssim_accum, adnm_hip.validate.Validator) on the
GPU: pinned by the reference's own evaluator fixture, compared with the kernels the accumulating pass shares its code with
(GpuEvaluator, ops.rainloss) at the shapes where an accumulating fold can go wrong, and run end to end beside a FlatTrainer."""
import ctypes

import numpy as np
import pytest
import torch

from adnm_hip import lib, ops, recipe
from util import load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR = [20, 30, 35, 40]
THR_SETS = {"one": [30], "default": THR, "eight": [5, 10, 20, 30, 35, 40, 50, 70]}
SHAPES = [(3, 5, 11, 11),      # hw = 121: less than one workgroup; the SSIM valid region is 1 x 1
          (2, 3, 17, 19),      # hw = 323: no multiple of 256 or of 4
          (4, 1, 16, 16),      # T = 1
          (1, 4, 8, 8),        # too small for the 11 x 11 window: no SSIM
          (2, 20, 64, 64)]     # the recipe's 20 frames, 16 SSIM tiles per frame
# The loss partial of a workgroup is an fp32 sum whose longest chain of additions is: the lane's trips through its frame
# (hw / 256 rounded up, <= 16 at these shapes: one workgroup per frame up to hw = 4096), + 6 (the wave's butterfly) + 2 (the four waves).
# The partials are folded in double and the quotient is rounded to fp32 once: 16 + 6 + 2 + 1 = 25 roundings, plus the few ulp of __expf
# in a term.  Every term is non-negative, so the relative error of the sum is below (chain) * 2^-24; the bar is 256 * 2^-24.
LOSS_BOUND = 256 * 2.0 ** -24


def _block(T, nthr):
    return torch.zeros(lib.query("adnm_valid_block_bytes", T, nthr) // 8, dtype=torch.float64, device=DEV)


def _accum(pred, tgt, block, thr, scale, loss=(0.57, 0.25, 0.0), ssim=True, loss_out=None):
    """the two entry points, called directly on (B, T, H, W) tensors"""
    B, T, H, W = pred.shape
    assert pred.is_contiguous() and tgt.is_contiguous() and pred.dtype == tgt.dtype == torch.float32
    thr_c = (ctypes.c_float * len(thr))(*thr)
    stream = torch.cuda.current_stream().cuda_stream
    nb = lib.query("adnm_valid_accum_ws_bytes", B * T, T, H * W, len(thr))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    lib.call("adnm_valid_accum", pred.data_ptr(), tgt.data_ptr(), block.data_ptr(), None if loss_out is None else loss_out.data_ptr(), thr_c, len(thr),
             float(scale), loss[0], loss[1], loss[2], ws.data_ptr(), nb, B * T, T, H * W, stream)
    if ssim and H > 10 and W > 10:
        nb2 = lib.query("adnm_valid_ssim_accum_ws_bytes", B * T, T, H, W, len(thr))
        ws2 = torch.empty(nb2, dtype=torch.uint8, device=DEV)
        lib.call("adnm_valid_ssim_accum", pred.data_ptr(), tgt.data_ptr(), block.data_ptr(), len(thr), float(scale), ws2.data_ptr(), nb2, B * T, T, H, W, stream)
    torch.cuda.synchronize()


def _pair(shape, salt=0):
    """prediction and target in [-1.2, 1.2): values below 0 and above 1 (the clip matters), targets on both sides of 0.7"""
    name = "validate." + "x".join(map(str, shape))
    return recipe.tensor(name + ".pred", shape, scale=1.2, salt=salt).to(DEV), recipe.tensor(name + ".tgt", shape, scale=1.2, salt=salt).to(DEV)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _same_result(a, b):
    """two done() dictionaries, NaN-safe (a score is 0 / 0 where nothing crosses a threshold)"""
    return repr(a) == repr(b)


# ------------------------------------------------------------------------------------------------ 1. pinned by the reference
def test_entry_points_vs_reference_fixture():
    from adnm_hip.validate import aggregate
    z = load_npz("evaluator_b3_t5")
    scale = float(z["value_scale"])
    t, p = z["truth"].to(DEV), z["pred"].to(DEV)
    blk = _block(5, 4)
    _accum(p[:2].contiguous(), t[:2].contiguous(), blk, THR, scale)
    _accum(p[2:].contiguous(), t[2:].contiguous(), blk, THR, scale)
    res = aggregate(blk.cpu().numpy(), THR, 5, 48 * 48, 38 * 38)
    assert (res["batches"], res["samples"], res["nonfinite"]) == (2, 3, 0)
    for thr in THR:
        m = res["threshold_metrics"][thr]
        for k in ("TP", "TN", "FP", "FN"):
            assert m[k] == float(z[f"{k}.{thr}"]), (thr, k)
        for k in ("CSI", "POD", "HSS"):
            assert abs(m[k] - float(z[f"{k}.{thr}"])) <= 1e-9, (thr, k)
    print("FAR", res["FAR"], float(z["FAR"]), "SSIM", res["SSIM"], float(z["SSIM"]), "RMSE", res["RMSE"], float(z["RMSE"]), "MSE", res["MSE"], float(z["mse"].mean()))
    assert abs(res["FAR"] - float(z["FAR"])) <= 1e-9
    assert abs(res["SSIM"] - float(z["SSIM"])) <= 1e-6, (res["SSIM"], float(z["SSIM"]))
    assert abs(res["RMSE"] - float(z["RMSE"])) <= 1e-5 * float(z["RMSE"])
    assert abs(res["MSE"] - float(z["mse"].mean())) <= 1e-5 * float(z["mse"].mean())


# ------------------------------------------------------------------------------------------------ 2. against the parent's kernels
@pytest.mark.parametrize("thr_name", list(THR_SETS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_table_vs_gpu_evaluator(shape, thr_name):
    from adnm_hip.evaluator import GpuEvaluator
    thr, scale = THR_SETS[thr_name], 90.0
    B, T, H, W = shape
    n = len(thr)
    pred, tgt = _pair(shape)
    ev = GpuEvaluator(T, scale, thr)
    ev.evaluate(tgt, pred)
    ref = ev._tables[0][0].double().cpu().numpy()          # (B, T, 4n + 2): per (sample, frame index)
    blk = _block(T, n)
    _accum(pred, tgt, blk, thr, scale)
    _accum(pred, tgt, blk, thr, scale)                     # the block ACCUMULATES: a second batch of the same data doubles it
    host = blk.cpu().numpy()
    tab = host[4:].reshape(T, 4 * n + 3)
    assert host[1] == 2 and host[2] == 2 * B and host[3] == 0
    want = 2 * ref.sum(0)                                   # summed over the samples per frame index t
    assert (tab[:, :4 * n] == want[:, :4 * n]).all(), "contingency counts differ from adnm_eval_counts"
    assert tab[:, :4 * n].sum() == 2.0 * n * B * T * H * W
    ra, rq = _rel(tab[:, 4 * n], want[:, 4 * n]), _rel(tab[:, 4 * n + 1], want[:, 4 * n + 1])
    print(f"{shape} {thr_name}: sum|d| rel {ra:.2e}, sum d^2 rel {rq:.2e}")
    assert ra <= 1e-6 and rq <= 1e-6
    if H > 10 and W > 10:
        sref = 2 * ev._ssim[0][0].double().cpu().numpy().sum(0)
        rs = _rel(tab[:, 4 * n + 2], sref)
        print(f"{shape} {thr_name}: SSIM sums rel {rs:.2e}")
        assert rs <= 1e-6
    else:
        assert ev._ssim[0][0] is None and (tab[:, 4 * n + 2] == 0).all()
    if B > 1 and T > 1:
        # distinct data per sample: frame f belongs to row f mod T; taking f / T instead groups other frames
        wrong = 2 * ref.reshape(B * T, -1)[:, :4 * n].reshape(T, B, -1).sum(1)
        assert not (wrong == want[:, :4 * n]).all(), "the two groupings coincide on this data: nothing is tested"
        assert not (tab[:, :4 * n] == wrong).all()


# ------------------------------------------------------------------------------------------------ 3. the loss
@pytest.mark.parametrize("gamma", [0.0, 0.1])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[4]], ids=lambda s: "x".join(map(str, s)))
def test_loss_value(shape, gamma):
    from models.loss import enRainfallLoss
    crit = enRainfallLoss(0.57, 0.25, gamma)
    B, T, H, W = shape
    blk, out = _block(T, 4), torch.zeros((), dtype=torch.float32, device=DEV)
    got, want_sum = [], 0.0
    for salt in range(3):
        pred, tgt = _pair(shape, salt)
        fp, ft = pred.view(-1), tgt.view(-1)
        fp[3:40:9] = ft[3:40:9]                       # pred == target: the sign of a zero difference, `over` on equality
        ft[50:90:8] = 0.7                             # target == 0.7f exactly: the heavy-rain threshold is `>=`
        ft[51], fp[51] = 0.7, 0.7
        assert int((ft == 0.7).sum()) >= 6 and int((fp == ft).sum()) >= 5 and int((ft > 0.7).sum()) > 0 and int(((ft >= 0.7) & (fp < ft)).sum()) > 0
        _accum(pred, tgt, blk, THR, 90.0, loss=(0.57, 0.25, gamma), ssim=False, loss_out=out)
        v = out.item()
        # fp64 on the CPU.  The reference decides `target >= 0.7` in fp32, where 0.7 IS the fp32 value nearest to it; widened to
        # double that value lies 1.2e-8 below the double 0.7 and would fall on the other side, so those elements (and only those)
        # are handed to the checker as the double 0.7: a 1.7e-8 relative change of their terms, far below the bar.
        t64 = tgt.double().cpu()
        t64[tgt.cpu() == 0.7] = 0.7
        want = float(crit.forward_torch(pred.double().cpu(), t64))
        plain = float(crit(pred, tgt))               # ops.rainloss on the same inputs
        print(f"{shape} gamma {gamma} batch {salt}: valid_accum {v!r}, fp64 {want!r} (rel {abs(v - want) / want:.2e}), rainloss {plain!r} (rel {abs(v - plain) / want:.2e})")
        assert abs(v - want) <= LOSS_BOUND * want
        assert abs(v - plain) <= 2 * LOSS_BOUND * want
        got.append(v)
        want_sum += float(np.float64(np.float32(v)))
    host = blk.cpu().numpy()
    assert host[0] == want_sum == sum(got), "loss_sum is not the double sum of the three fp32 batch losses"
    assert host[1] == 3 and host[2] == 3 * B and host[3] == 0


# ------------------------------------------------------------------------------------------------ 4. / 5.
def test_a_nan_batch_is_counted_and_adds_no_loss():
    shape = (2, 3, 17, 19)
    pred, tgt = _pair(shape)
    blk = _block(3, 4)
    _accum(pred, tgt, blk, THR, 90.0)
    before = blk.cpu().numpy().copy()
    bad = pred.clone()
    bad[1, 2, 5, 7] = float("nan")
    out = torch.zeros((), dtype=torch.float32, device=DEV)
    _accum(bad, tgt, blk, THR, 90.0, loss_out=out)
    host = blk.cpu().numpy()
    assert np.isnan(out.item())
    assert host[3] == 1 and host[1] == 2 and host[2] == 4
    assert host[0] == before[0] and np.isfinite(host[0]) and host[0] > 0
    assert np.isfinite(host).all(), "the NaN reached the table (the clip turns it into 0 as fmaxf does in adnm_eval_counts)"


def test_two_runs_give_the_same_bits():
    shape = (2, 20, 64, 64)
    batches = [_pair(shape, salt) for salt in (0, 1)]
    blocks = []
    for _ in range(2):
        blk = _block(20, 4)
        for pred, tgt in batches:
            _accum(pred, tgt, blk, THR, 90.0, loss=(0.57, 0.25, 0.1))
        blocks.append(blk)
    assert float(blocks[0][0]) > 0 and float(blocks[0][4:].abs().sum()) > 0
    assert torch.equal(blocks[0].view(torch.int64), blocks[1].view(torch.int64))


# ------------------------------------------------------------------------------------------------ 6. the Validator end to end
def _model(salt=0):
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(m, salt=salt)
    return m.to(DEV).train()


_data = {}


def _batches():
    if "b" not in _data:
        frames = recipe.radar_batch(10, 25, 64, name="validate.e2e").to(DEV)
        _data["b"] = [(frames[i:i + 2, :5].contiguous(), frames[i:i + 2, 5:].contiguous()) for i in range(0, 10, 2)]
    return _data["b"]


def test_validator_end_to_end():
    from adnm_hip.evaluator import GpuEvaluator, GraphedForward
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    model, crit, scale = _model().eval(), enRainfallLoss(0.57, 0.25, gamma=0.0), 255.0
    data = _batches()[:2]
    # the route of the parent commit: the graphed forward, the loss with its .item(), the evaluator's tables per batch
    fwd, ev, loss_sum = GraphedForward(model), GpuEvaluator(20, scale, THR), 0.0
    for x, tgt in data:
        out = fwd(x)
        loss_sum += crit(out, tgt).item()
        ev.evaluate(tgt, out)
    ref = ev.done()
    fwd.close()
    val = Validator(model, crit, 20, scale, THR)
    try:
        for x, tgt in data:
            val.step(x, tgt)
        res = val.done(reset=True)
        assert float(val._block.abs().sum()) == 0.0, "done(reset=True) left something in the block"
        assert set(res) == set(ref) | {"loss_sum", "loss_mean", "batches", "samples", "nonfinite"}
        assert (res["batches"], res["samples"], res["nonfinite"]) == (2, 4, 0) and res["LPIPS"] is None
        print("validator", {k: v for k, v in res.items() if k != "threshold_metrics"}, "parent route", {k: v for k, v in ref.items() if k != "threshold_metrics"}, loss_sum)
        for thr in THR:
            a, b = res["threshold_metrics"][thr], ref["threshold_metrics"][thr]
            for k in ("TP", "TN", "FP", "FN"):
                assert a[k] == b[k], (thr, k, a[k], b[k])
            for k in ("CSI", "POD", "HSS"):
                assert (np.isnan(a[k]) and np.isnan(b[k])) or abs(a[k] - b[k]) <= 1e-9, (thr, k)
        assert sum(res["threshold_metrics"][20][k] for k in ("TP", "TN", "FP", "FN")) == 4 * 20 * 64 * 64
        assert (np.isnan(res["FAR"]) and np.isnan(ref["FAR"])) or abs(res["FAR"] - ref["FAR"]) <= 1e-9
        for k in ("RMSE", "MAE", "MSE", "SSIM"):
            assert abs(res[k] - ref[k]) <= 1e-6 * abs(ref[k]), (k, res[k], ref[k])
        assert abs(res["loss_sum"] - loss_sum) <= 2 * LOSS_BOUND * loss_sum and res["loss_mean"] == res["loss_sum"] / 2
        # a second epoch on the same batches: the same bits; and no allocation once the graph exists
        for x, tgt in data:
            val.step(x, tgt)
        again = val.done(reset=True)
        assert _same_result(again, res), (again, res)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        for x, tgt in (data + data)[:3]:
            val.step(x, tgt)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        assert val.done()["batches"] == 3
    finally:
        val.close()


# ------------------------------------------------------------------------------------------------ 7. beside a FlatTrainer
FP8_PERIOD = 2   # instead of 16: the record flags of the delayed-scaling table are SET while the second validation epoch runs


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


def _trainer(model):
    from adnm_hip.trainer import FlatTrainer
    from models.loss import enRainfallLoss
    return FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025, use_graph=True)


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


def _train(prec, validate):
    """3 steps; validate: a 2-batch validation epoch after step 1 and after step 2.  -> (trainer state, model state[, results, check])"""
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    data = _batches()
    ops.QUANT.reset()
    model = _model()
    tr = _trainer(model)
    val = Validator(model, enRainfallLoss(0.57, 0.25, gamma=0.0), 20, 255.0, THR) if validate else None
    results = []
    try:
        for i in range(3):
            tr.step(*data[i])
            if validate and i < 2:
                for x, tgt in data[3:5]:
                    val.step(x, tgt)
                results.append(val.done(reset=True))
        state = tr.state_dict()
        params = {k: v.detach().to("cpu", copy=True) for k, v in model.state_dict().items()}
        check = None
        if validate:
            x, tgt = data[3]
            out = val.step(x, tgt).clone()          # after step 3: it must have read the CURRENT narrow shadow
            model.eval()
            with torch.no_grad():
                eager = model(x)
            model.train()
            torch.cuda.synchronize()
            check = (out, eager)
        return state, params, results, check
    finally:
        if val is not None:
            val.close()
        tr.close()


@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_validation_does_not_perturb_training(prec):
    with _Precision(prec):
        plain = _train(prec, False)
        mixed = _train(prec, True)
    _same(mixed[0], plain[0], "trainer state (moments, state, fp8: the quantisation table) after 3 steps with validation in between")
    _same(mixed[1], plain[1], "parameters after 3 steps with validation in between")
    if prec == "fp8":
        rows = plain[0]["fp8"]["rows"]
        assert len(rows) > 50 and bool((torch.stack([v[:2] for v in rows.values()]) != 1.0).any()), "no record ever made a scale: nothing is tested"
    r1, r2 = mixed[2]
    assert r1["batches"] == r2["batches"] == 2 and r1["nonfinite"] == r2["nonfinite"] == 0
    assert r1["loss_sum"] != r2["loss_sum"], "the second validation epoch saw the weights of the first: a stale shadow"
    out, eager = mixed[3]
    assert torch.equal(out, eager), "the Validator's forward after step 3 is not the eager forward on the current weights"


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals():
    from adnm_hip.validate import Validator
    from models.loss import RainfallLoss, Weighted_mse_mae, enRainfallLoss
    model = torch.nn.Identity()
    with pytest.raises(RuntimeError, match="enRainfallLoss"):
        Validator(model, Weighted_mse_mae(), 20, 255.0)
    with pytest.raises(RuntimeError, match="enRainfallLoss"):
        Validator(model, torch.nn.L1Loss(), 20, 255.0)
    with pytest.raises(ValueError):
        Validator(model, enRainfallLoss(), 20, 255.0, thresholds=())
    val = Validator(model, RainfallLoss(), 20, 255.0)
    x, tgt = torch.zeros(2, 20, 1, 16, 16), torch.zeros(2, 20, 1, 16, 16)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        val.step(x, tgt)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        val.step(x.to(DEV), tgt)
    with pytest.raises(RuntimeError, match="seq_len is 20"):
        val.step(x.to(DEV), torch.zeros(2, 19, 1, 16, 16, device=DEV))
    with pytest.raises(RuntimeError, match="no batch"):
        val.done()
    # and the accepted case on the same object: an identity "model" whose output is the input (a perfect forecast)
    val.step(x.to(DEV) + 0.5, tgt.to(DEV) + 0.5)
    res = val.done()
    assert res["loss_sum"] == 0.0 and res["MSE"] == 0.0 and res["samples"] == 2 and abs(res["SSIM"] - 1.0) <= 1e-12
    val.close()

    # a model whose output does not match the target: refused on the warm-up forward's output, before any capture
    class FirstFrames(torch.nn.Module):
        t = 19

        def forward(self, x):
            return x[:, :self.t]

    short = FirstFrames()
    val = Validator(short, RainfallLoss(), 20, 255.0)
    with pytest.raises(RuntimeError, match="does not match the target"):
        val.step(x.to(DEV), tgt.to(DEV))
    assert not torch.cuda.is_current_stream_capturing()
    assert float(val._block.abs().sum()) == 0.0
    short.t = 20
    val.step(x.to(DEV), tgt.to(DEV))
    assert val.done()["batches"] == 1
    val.close()
