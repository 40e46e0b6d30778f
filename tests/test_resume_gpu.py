"""Stop and go on, on the GPU (FlatTrainer.state_dict / load_state_dict / snapshot, checkpoint.save_training_state /
load_training_state): ADNM-UNet 5 -> 20 at 64 x 64, B = 2, hipGraph steps.  A run that saves after step 2, dies, and goes on in a new
trainer built on a differently initialised model must hold after step 4 the bits the uninterrupted twin holds — parameters, moments,
`state`, the loss of steps 3 and 4, in fp8 the quantisation records — and a load into a prepared trainer must leave its graphs valid."""
import pytest
import torch

from adnm_hip import checkpoint, ops, recipe
from adnm_hip.trainer import FlatTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECS = ["f32", "bf16", "fp8"]
FP8_PERIOD = 2   # instead of 16: steps 2 and 4 of these runs end a recording step and make new scales, so the table really moves


def _model(salt=0):
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(m, salt=salt)
    return m.to(DEV).train()


def _trainer(model, **kw):
    from models.loss import enRainfallLoss
    kw.setdefault("lr", 1e-3)
    return FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                       use_graph=True, **kw)


_data = {}


def _batches():
    if "b" not in _data:
        frames = recipe.radar_batch(8, 25, 64, name="resume").to(DEV)
        _data["b"] = [(frames[i:i + 2, :5].contiguous(), frames[i:i + 2, 5:].contiguous()) for i in range(0, 8, 2)]
    return _data["b"]


def _poisoned(x):
    """one inf pixel (tests/test_step_guard_gpu.py): the gradient of every parameter becomes non-finite"""
    x = x.clone()
    x[0, 2, 0, 31, 17] = float("inf")
    return x


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)


def _same(a, b, what=""):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what} differs"
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


def _model_state(model):
    return {k: v.detach().to("cpu", copy=True).contiguous() for k, v in model.state_dict().items()}


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


_twins = {}


def _twin(prec, **kw):
    """the uninterrupted run: 4 steps; trainer state and model after steps 2 and 4, the four losses.  Call inside _Precision(prec).
    The plain f32 and bf16 twins serve several tests and are made once (0.9 GB of host memory per kept state: the others are not kept)."""
    key = (prec, tuple(sorted(kw.items())))
    if key in _twins:
        return _twins[key]
    poison = kw.pop("poison", False)
    model = _model(0)
    tr = _trainer(model, **kw)
    out = {"loss": []}
    try:
        for i, (x, t) in enumerate(_batches(), start=1):
            out["loss"].append(float(tr.step(_poisoned(x) if (poison and i == 2) else x, t)))
            if i in (2, 4):
                out[i] = (tr.state_dict(), _model_state(model))
        if tr.monitor:
            out["stats"] = tr.stats()
    finally:
        tr.close()
    if prec in ("f32", "bf16") and not key[1]:
        _twins[key] = out
    return out


def _stats_same(a, b):
    """two stats() dicts, NaN-safe (the last norm of a skipped step is inf or nan)"""
    return a.keys() == b.keys() and all(repr(a[k]) == repr(b[k]) for k in a)


def _nhwc_case(tr):
    """(index, name) of a dense-conv weight that the flat buffers hold channels-last and for which that order differs from NCHW"""
    name_of = {id(p): n for n, p in tr.model.named_parameters()}
    for i, p in enumerate(tr.used):
        if p.dim() == 4 and not p.is_contiguous() and p.shape[1] > 1 and p.shape[2] * p.shape[3] > 1:
            return i, name_of[id(p)]
    raise AssertionError("no channels-last conv weight among the used parameters")


@pytest.mark.parametrize("prec", PRECS)
def test_bit_exact_resume(prec, tmp_path):
    data = _batches()
    path = str(tmp_path / "state.pth")
    with _Precision(prec):
        a = _twin(prec)
        ops.QUANT.reset()
        b = _trainer(_model(0))
        try:
            for x, t in data[:2]:
                b.step(x, t)
            assert b.shadow_mode == PRECS.index(prec) and b.graph is not None
            checkpoint.save_training_state(b, path)
        finally:
            b.close()
        del b
        ops.QUANT.reset()
        model = _model(1)   # other weights
        tr = _trainer(model, lr=0.5)
        try:
            tr.prepare(*data[3])
            ptrs = [t.data_ptr() for t in (tr.flat_p, tr.flat_g, tr.exp_avg, tr.exp_avg_sq, tr.state)]
            assert checkpoint.load_training_state(tr, path) is None
            assert ptrs == [t.data_ptr() for t in (tr.flat_p, tr.flat_g, tr.exp_avg, tr.exp_avg_sq, tr.state)] and tr.lr == 1e-3
            _same(tr.state_dict(), a[2][0], "state right after the load")
            _same(_model_state(model), a[2][1], "model right after the load")
            if prec == "bf16":
                assert torch.equal(tr.shadow, tr.flat_p.to(torch.bfloat16)) and not tr._shadow.stale()
            if prec == "fp8":
                rows = a[2][0]["fp8"]["rows"]
                assert len(rows) > 50 and any(k.endswith("|w") for k in rows) and any(k.endswith("|fnt") for k in rows)
                assert any(k.endswith("|gnn") for k in rows), sorted({k.split("|")[1] for k in rows})
                scales = torch.stack([v[:2] for v in rows.values()])
                assert bool((scales != 1.0).any()), "no record ever made a scale: the fp8 case checks nothing"
                assert not tr._shadow.stale()
            losses = [float(tr.step(x, t)) for x, t in data[2:]]
            print(f"{prec}: losses of the twin {a['loss']}, of the resumed run {losses}")
            assert losses == a["loss"][2:], (losses, a["loss"])
            _same(tr.state_dict(), a[4][0], "state after steps 3-4")     # moments, state, fp8: the table's rows and its state pair
            _same(_model_state(model), a[4][1], "model after steps 3-4")   # flat_p through the parameters
            if prec == "fp8":
                assert not torch.equal(torch.stack(list(a[4][0]["fp8"]["rows"].values())), torch.stack(list(a[2][0]["fp8"]["rows"].values())))
        finally:
            tr.close()


def test_layouts_and_a_load_into_a_prepared_staged_trainer():
    """the unstaged twin's state into a prepared 5-stage trainer (name-keyed: another order, other bucket padding, the same
    channels-last conv weights); then the staged twin's state, and two replayed steps against that twin"""
    data = _batches()
    with _Precision("f32"):
        plain = _twin("f32")
        staged = _twin("f32", overlap=True)
        model = _model(1)
        tr = _trainer(model, overlap=True)
        try:
            tr.prepare(*data[0])
            assert tr.staged and len(tr.buckets) == 5 and len(tr.graphs) == 4 and tr.tail is not None
            ptrs = [t.data_ptr() for t in (tr.flat_p, tr.flat_g, tr.exp_avg, tr.exp_avg_sq, tr.state, tr.hyper)]
            graphs = [id(g) for g in tr.graphs] + [id(tr.graph), id(tr.tail)]
            assert list(plain[2][0]["params"]) != tr._used_names(), "the two layouts order the parameters alike: nothing is tested"
            model.load_state_dict(plain[2][1])
            tr.load_state_dict(plain[2][0])
            got = tr.state_dict()
            _same(got, plain[2][0], "unstaged -> 5 stages")
            i, name = _nhwc_case(tr)
            p, o = tr.used[i], tr.offs[i]
            co, ci, kh, kw = p.shape
            for key, buf in (("exp_avg", tr.exp_avg), ("exp_avg_sq", tr.exp_avg_sq)):
                saved = got["params"][name][key]
                assert saved.shape == p.shape and saved.is_contiguous()
                raw = buf[o:o + p.numel()].cpu()
                assert torch.equal(saved, raw.view(co, kh, kw, ci).permute(0, 3, 1, 2)), f"{name}: {key} did not come back in NCHW"
                assert not torch.equal(saved.flatten(), raw), f"{name}: channels-last and NCHW coincide: choose another weight"
            model.load_state_dict(staged[2][1])
            tr.load_state_dict(staged[2][0])
            assert ptrs == [t.data_ptr() for t in (tr.flat_p, tr.flat_g, tr.exp_avg, tr.exp_avg_sq, tr.state, tr.hyper)]
            assert graphs == [id(g) for g in tr.graphs] + [id(tr.graph), id(tr.tail)] and len(tr.graphs) == 4
            losses = [float(tr.step(x, t)) for x, t in data[2:]]
            assert losses == staged["loss"][2:], (losses, staged["loss"])
            _same(tr.state_dict(), staged[4][0], "state after two replayed steps")
            _same(_model_state(model), staged[4][1], "model after two replayed steps")
        finally:
            tr.close()
        # and the other direction: the staged twin's state into an unstaged trainer that has not been prepared yet
        model = _model(1)
        tr = _trainer(model)
        try:
            model.load_state_dict(staged[2][1])
            tr.load_state_dict(staged[2][0])
            assert tr.used is None
            tr.prepare(*data[0])   # the tail-less single graph; the warm-ups must not have touched what was loaded
            assert not tr.staged
            _same(tr.state_dict(), staged[2][0], "5 stages -> unstaged, loaded before prepare()")
            _same(_model_state(model), staged[2][1], "model after prepare()")
        finally:
            tr.close()


def test_monitor_statistics_survive_the_restart(tmp_path):
    data = _batches()
    path = str(tmp_path / "state.pth")
    with _Precision("f32"):
        a = _twin("f32", monitor=True, poison=True)
        assert a["stats"]["skipped"] == 1 and a["stats"]["steps"] == 3, a["stats"]
        b = _trainer(_model(0), monitor=True)
        try:
            b.step(*data[0])
            b.step(_poisoned(data[1][0]), data[1][1])
            half = b.stats()
            assert half["skipped"] == 1 and half["steps"] == 1
            checkpoint.save_training_state(b, path, schedule_stats=half)
        finally:
            b.close()
        model = _model(1)
        tr = _trainer(model, monitor=True)
        try:
            tr.prepare(*data[0])
            assert _stats_same(checkpoint.load_training_state(tr, path), half)
            assert _stats_same(tr.stats(), half), (tr.stats(), half)
            for x, t in data[2:]:
                tr.step(x, t)
            st = tr.stats()
            assert _stats_same(st, a["stats"]) and st["skipped"] == 1 and st["steps"] == 3, (st, a["stats"])
            _same(tr.state_dict(), a[4][0], "monitored run after the restart")
        finally:
            tr.close()


def test_snapshot_is_consistent_and_does_not_wait():
    data = _batches()
    with _Precision("f32"):
        a = _twin("f32")
        model = _model(0)
        tr = _trainer(model)
        try:
            for x, t in data[:2]:
                tr.step(x, t)
            snap = tr.snapshot()
            for x, t in data[2:]:     # enqueued behind the snapshot's copies, no synchronisation in between
                tr.step(x, t)
            sd = snap.state_dict()
            params = sd.pop("parameters")
            _same(sd, a[2][0], "snapshot after step 2")
            assert set(params) == set(sd["params"])
            for n, v in params.items():
                assert v.is_contiguous() and torch.equal(_bits(v), _bits(a[2][1][n])), f"parameter {n} of the snapshot"
            _same(tr.state_dict(), a[4][0], "the trainer itself after steps 3-4")
            _same(_model_state(model), a[4][1], "the model itself after steps 3-4")
        finally:
            tr.close()


def test_graphed_forward_after_a_load(tmp_path):
    from adnm_hip.evaluator import GraphedForward
    data = _batches()
    x = data[3][0]
    with _Precision("bf16"):
        a = _twin("bf16")
        blob = {"format": checkpoint.TRAINING_STATE, "version": 1, "model": a[2][1], "trainer": a[2][0], "schedule_stats": None}
        # a model that held those weights from the start
        ref_model = _model(1)
        ref_model.load_state_dict(a[2][1])
        ref_tr = _trainer(ref_model)
        try:
            ref_tr.prepare(*data[0])
            ref_fwd = GraphedForward(ref_model)
            ref = ref_fwd(x).clone()
            torch.cuda.synchronize()
            ref_fwd.close()
        finally:
            ref_tr.close()
        model = _model(1)
        tr = _trainer(model)
        try:
            tr.step(*data[0])
            fwd = GraphedForward(model)
            before = fwd(x).clone()       # captured on the other weights
            checkpoint.load_training_state(tr, blob)
            out = fwd(x).clone()
            torch.cuda.synchronize()
            assert not torch.equal(before, ref)
            assert torch.equal(out, ref), "GraphedForward after load_training_state does not compute with the loaded weights"
            fwd.close()
        finally:
            tr.close()
