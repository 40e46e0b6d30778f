"""FlatTrainer(ema_decay=...) on the GPU: ADNM-UNet 5 -> 20 at 64 x 64, B = 2, hipGraph steps (the shape of tests/test_resume_gpu.py).
The average never touches the training run, follows its recurrence step by step, stands still on skipped steps and inside an
accumulation cycle, can be computed with (ema_weights()) and put back bit for bit, and survives a restart."""
import pytest
import torch

from adnm_hip import checkpoint, ops, recipe
from adnm_hip.trainer import FlatTrainer
from ema_ref import assert_ema_step, warmup_decay

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECS = ["f32", "bf16", "fp8"]
DECAY = 0.999
EMA_KEYS = {"ema", "ema_info", "ema_decay", "ema_warmup"}
PLAIN_KEYS = {"version", "precision", "steps", "lr", "max_norm", "betas", "eps", "weight_decay", "accum_steps", "micro_step", "state_bits",
              "params", "monitor", "fp8"}


def _model(salt=0):
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(m, salt=salt)
    return m.to(DEV).train()


def _crit():
    from models.loss import enRainfallLoss
    return enRainfallLoss(0.57, 0.25, gamma=0.0)


def _trainer(model, **kw):
    return FlatTrainer(model, _crit(), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025, use_graph=True, **kw)


_data = {}


def _batches():
    if "b" not in _data:
        frames = recipe.radar_batch(10, 25, 64, name="resume").to(DEV)
        _data["b"] = [(frames[i:i + 2, :5].contiguous(), frames[i:i + 2, 5:].contiguous()) for i in range(0, 10, 2)]
    return _data["b"]


def _poisoned(x):
    """one inf pixel (tests/test_step_guard_gpu.py): the gradient of every parameter becomes non-finite"""
    x = x.clone()
    x[0, 2, 0, 31, 17] = float("inf")
    return x


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same(a, b, what=""):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and _eq(a, b), f"{what} differs"
    elif isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), f"{what}: keys differ: {sorted(set(a) ^ set(b))[:6]}"
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        assert a == b, f"{what}: {a!r} vs {b!r}"


class _Precision:
    def __init__(self, prec):
        self.prec = prec

    def __enter__(self):
        ops.set_mfma_precision(self.prec)
        ops.QUANT.reset()

    def __exit__(self, *exc):
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()
        return False


def _device_state(tr):
    """clones of everything a training run is made of on the device: flat buffers, state, shadow, (fp8) the quantisation table"""
    d = {"flat_p": tr.flat_p.clone(), "exp_avg": tr.exp_avg.clone(), "exp_avg_sq": tr.exp_avg_sq.clone(), "state": tr.state.clone(),
         "shadow": None if tr.shadow is None else tr.shadow.clone()}
    if tr.fp8:
        d["qtab"], d["qstate"] = ops.QUANT.snapshot(tr.flat_p.device)
    return d


def _run_plain(nsteps, **kw):
    """a trainer WITHOUT the average: losses and the device state after nsteps.  Inside _Precision."""
    tr = _trainer(_model(0), **kw)
    try:
        losses = [float(tr.step(x, t)) for x, t in _batches()[:nsteps]]
        assert tr.ema is None and tr._ema_info is None
        return losses, _device_state(tr), set(tr.state_dict()) if nsteps == 1 else None
    finally:
        tr.close()


# the captured tail graph (5 stages: overlap=True) for f32 and fp8, the eager tail of the single graph for bf16
@pytest.mark.parametrize("prec,overlap", [("f32", True), ("bf16", False), ("fp8", True)])
def test_average_is_read_only_on_training_and_obeys_its_recurrence(prec, overlap):
    data = _batches()
    with _Precision(prec):
        losses, want, _ = _run_plain(4, overlap=overlap)
        ops.QUANT.reset()
        tr = _trainer(_model(0), overlap=overlap, ema_decay=DECAY)
        try:
            tr.prepare(*data[0])
            assert (tr.tail is not None) == overlap and tr.shadow_mode == PRECS.index(prec)
            assert _eq(tr.ema, tr.flat_p) and tr.ema.data_ptr() != tr.flat_p.data_ptr(), "the average does not start as a copy of the parameters"
            assert tr.ema_info() == {"decay": 0.0, "updates": 0}, "prepare()'s tail warm-up left its update behind"
            got = []
            for i, (x, t) in enumerate(data[:4], start=1):
                before = tr.ema.clone()
                got.append(float(tr.step(x, t)))
                info = tr.ema_info()
                assert info["updates"] == i, info
                ramp = warmup_decay(DECAY, i)
                assert abs(info["decay"] - ramp) <= 4 * 2.0 ** -24 * ramp, (i, info, ramp)
                assert_ema_step(tr.ema, before, tr.flat_p, info["decay"], f"{prec}: step {i}")
                assert not _eq(tr.ema, before) and not _eq(tr.ema, tr.flat_p)
            assert got == losses, (got, losses)
            _same(_device_state(tr), want, f"{prec}: training state beside a twin without the average")
        finally:
            tr.close()


@pytest.mark.parametrize("overlap", [False, True])
def test_skipped_step_leaves_the_average_alone(overlap):
    data = _batches()
    with _Precision("bf16"):
        tr = _trainer(_model(0), overlap=overlap, monitor=True, ema_decay=DECAY)
        try:
            tr.step(*data[0])
            ema1, info1, raw1 = tr.ema.clone(), tr.ema_info(), tr._ema_info.clone()
            assert info1["updates"] == 1
            tr.step(_poisoned(data[1][0]), data[1][1])
            assert tr.stats()["skipped"] == 1
            assert _eq(tr.ema, ema1) and _eq(tr._ema_info, raw1), "a skipped step moved the average or its counters"
            tr.step(*data[2])
            info3 = tr.ema_info()
            assert info3["updates"] == 2 and tr.stats()["skipped"] == 1 and tr.stats()["steps"] == 2
            ramp = warmup_decay(DECAY, 2)   # the device's step counter stood still on the skipped step
            assert abs(info3["decay"] - ramp) <= 4 * 2.0 ** -24 * ramp, (info3, ramp)
            assert_ema_step(tr.ema, ema1, tr.flat_p, info3["decay"], "the step after the skip")
        finally:
            tr.close()


def test_accumulation_moves_the_average_once_per_cycle():
    data = _batches()
    with _Precision("f32"):
        tr = _trainer(_model(0), accum_steps=2, ema_decay=DECAY)
        try:
            tr.prepare(*data[0])
            ema0 = tr.ema.clone()
            for cycle in (1, 2):
                tr.step(*data[2 * cycle - 2])
                assert tr.micro_step == 1 and _eq(tr.ema, ema0) and tr.ema_info()["updates"] == cycle - 1, "call 1 of a cycle moved the average"
                with pytest.raises(RuntimeError, match="accumulation cycle is open"):
                    with tr.ema_weights():
                        pass
                tr.step(*data[2 * cycle - 1])
                info = tr.ema_info()
                assert tr.micro_step == 0 and info["updates"] == cycle
                assert_ema_step(tr.ema, ema0, tr.flat_p, info["decay"], f"cycle {cycle}")
                assert not _eq(tr.ema, ema0)
                ema0 = tr.ema.clone()
        finally:
            tr.close()


def _forward(model, x):
    model.eval()
    with torch.no_grad():
        out = model(x).clone()
    model.train()
    return out


@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_ema_weights_computes_with_the_average_and_puts_the_run_back(prec):
    from adnm_hip.validate import Validator
    data = _batches()
    x, tgt = data[4]
    with _Precision(prec):
        losses, want, _ = _run_plain(5)   # the twin that never enters (the average is read-only: the test above)
        ops.QUANT.reset()
        model = _model(0)
        tr = _trainer(model, ema_decay=DECAY)
        val = Validator(model, _crit(), 20, 255.0)
        try:
            got = [float(tr.step(*b)) for b in data[:3]]
            val.step(x, tgt)                                   # captures the forward graph BEFORE the context, on the last-step weights
            loss_last = val.done(reset=True)["loss_sum"]
            before, ema_before = _device_state(tr), tr.ema.clone()
            with tr.ema_weights():
                assert _eq(tr.flat_p, ema_before) and _eq(tr.ema, before["flat_p"])
                assert not tr._shadow.stale()
                eager = _forward(model, x)
                graphed = val.step(x, tgt).clone()
                loss_avg = val.done(reset=True)["loss_sum"]
                averaged = {k: v.detach().to("cpu", copy=True).contiguous() for k, v in model.state_dict().items()}
                for what, call in (("step", lambda: tr.step(*data[3])), ("prepare", lambda: tr.prepare(*data[3])), ("snapshot", tr.snapshot),
                                   ("load_state_dict", lambda: tr.load_state_dict({})), ("ema_weights", lambda: tr.ema_weights().__enter__())):
                    with pytest.raises(RuntimeError, match="not inside ema_weights"):
                        call()
            _same(_device_state(tr), before, f"{prec}: the run after ema_weights()")
            assert _eq(tr.ema, ema_before) and not tr._shadow.stale()
            assert loss_avg != loss_last, "the validation loss under the average equals the last-step weights': the context changed nothing"
            with pytest.raises(ZeroDivisionError):
                with tr.ema_weights():
                    assert _eq(tr.flat_p, ema_before)
                    1 / 0
            _same(_device_state(tr), before, f"{prec}: the run after an exception inside ema_weights()")
            assert _eq(tr.ema, ema_before) and not tr._ema_open
            got += [float(tr.step(*b)) for b in data[3:5]]
            assert got == losses, (got, losses)
            _same(_device_state(tr), want, f"{prec}: two further steps beside a twin that never entered")
        finally:
            val.close()
            tr.close()
        # a second model that holds the averaged values through load_state_dict (the stale-shadow path rewrites its narrow shadow)
        ops.QUANT.reset()
        model2 = _model(0)
        tr2 = _trainer(model2)
        val2 = Validator(model2, _crit(), 20, 255.0)
        try:
            tr2.prepare(*data[0])
            model2.load_state_dict(averaged)
            assert tr2._shadow.stale()
            assert _eq(_forward(model2, x), eager), f"{prec}: eager forward under ema_weights() differs from a model holding the averaged weights"
            assert _eq(val2.step(x, tgt), graphed), f"{prec}: Validator.step under ema_weights() differs from a model holding the averaged weights"
            assert val2.done()["loss_sum"] == loss_avg
        finally:
            val2.close()
            tr2.close()


def _strip(sd):
    return {k: v for k, v in sd.items() if k not in EMA_KEYS}


@pytest.mark.parametrize("prec", PRECS)
def test_average_survives_a_restart_bit_for_bit(prec, tmp_path):
    data = _batches()
    path = str(tmp_path / "state.pth")
    with _Precision(prec):
        a = _trainer(_model(0), ema_decay=DECAY)
        try:
            for b in data[:2]:
                a.step(*b)
            checkpoint.save_training_state(a, path)
            for b in data[2:4]:
                a.step(*b)
            ema4, info4 = a.ema.clone(), a._ema_info.clone()
        finally:
            a.close()
        del a
        ops.QUANT.reset()
        tr = _trainer(_model(1), ema_decay=DECAY)   # other weights
        try:
            tr.prepare(*data[3])
            checkpoint.load_training_state(tr, path)
            assert tr.ema_info()["updates"] == 2
            for b in data[2:4]:
                tr.step(*b)
            assert _eq(tr.ema, ema4), f"{prec}: the average after the restart differs from the uninterrupted run's"
            assert _eq(tr._ema_info, info4), f"{prec}: ema_info after the restart differs"
        finally:
            tr.close()


def test_snapshot_layouts_and_the_load_cases():
    """snapshot() holds the average of the step it was taken behind; an unstaged run's state loads into a prepared 5-stage trainer
    (another order of the parameters, the same average by name); the strict / non-strict load cases of DESIGN.md §4g"""
    data = _batches()
    with _Precision("f32"):
        a = _trainer(_model(0), ema_decay=DECAY)
        try:
            for b in data[:2]:
                a.step(*b)
            snap = a.snapshot()
            sd2 = a.state_dict()
            a.step(*data[2])     # enqueued behind the snapshot's copies
            ssd = snap.state_dict()
            assert EMA_KEYS <= set(sd2) and set(sd2) - EMA_KEYS == PLAIN_KEYS
            _same(ssd["ema"], sd2["ema"], "snapshot: the average of the step it was taken behind")
            _same(ssd["ema_info"], sd2["ema_info"], "snapshot: ema_info")
            assert sd2["ema_decay"] == DECAY and sd2["ema_warmup"] is True and sd2["ema_info"].tolist()[1] == 2.0
            i = next(i for i, p in enumerate(a.used) if p.dim() == 4 and not p.is_contiguous() and p.shape[1] > 1 and p.shape[2] * p.shape[3] > 1)
            name = a._used_names()[i]
            saved = sd2["ema"][name]
            assert saved.is_contiguous() and saved.shape == a.used[i].shape   # logical NCHW, like the moments
            del snap, ssd
        finally:
            a.close()
        del a
        tr5 = _trainer(_model(1), overlap=True, ema_decay=DECAY)
        try:
            tr5.prepare(*data[0])
            assert tr5.staged and len(tr5.buckets) == 5 and list(sd2["ema"]) != tr5._used_names()
            seeded = tr5.ema.clone()
            with pytest.raises(RuntimeError, match="holds no 'ema'"):
                tr5.load_state_dict(_strip(sd2))
            assert _eq(tr5.ema, seeded)
            tr5.load_state_dict(sd2)
            names = tr5._used_names()
            host = tr5.ema.cpu()
            for i, n in enumerate(names):
                assert torch.equal(_bits(tr5._logical(host, i)), _bits(sd2["ema"][n])), f"unstaged -> 5 stages: ema of {n}"
            assert _eq(tr5._ema_info.cpu(), sd2["ema_info"])
            assert not _eq(tr5.ema, tr5.flat_p)
            tr5.load_state_dict(_strip(sd2), strict=False)
            assert _eq(tr5.ema, tr5.flat_p) and tr5._ema_info.tolist() == [0.0, 0.0], "strict=False did not start the average anew"
        finally:
            tr5.close()
        off = _trainer(_model(1))   # (no buffers yet: the checks come before anything is kept)
        with pytest.raises(RuntimeError, match="built without"):
            off.load_state_dict(sd2)
        off.load_state_dict(sd2, strict=False)
        assert off.ema is None and off.ema_decay is None
        other = _trainer(_model(1), ema_decay=0.5, ema_warmup=False)
        with pytest.raises(RuntimeError, match="hyper-parameters differ.*ema_decay.*ema_warmup"):
            other.load_state_dict(sd2)
        other.load_state_dict(sd2, strict=False)
        assert other.ema_decay == 0.5 and other.ema_warmup is False


def test_default_is_off_and_writes_the_keys_it_always_wrote():
    with _Precision("f32"):
        _, _, keys = _run_plain(1)
    assert keys == PLAIN_KEYS, sorted(keys ^ PLAIN_KEYS)
