"""Stop and go on, without a GPU: FlatTrainer.state_dict() / load_state_dict() and checkpoint.save_training_state /
load_training_state / to_torch_adamw_state / from_torch_adamw_state on the torch-ops path (fused=False).  Everything is compared on
bits: a resumed run must BE the uninterrupted one."""
import pytest
import torch
import torch.nn as nn

from adnm_hip import checkpoint, ops
from adnm_hip.trainer import FlatTrainer
from util import assert_close

HYPER = dict(lr=1e-2, eps=1e-9, weight_decay=1e-2, max_norm=0.5)


class Toy(nn.Module):
    """tests/test_ddp_gloo.py's Toy with a seed: two stages (forward_stage1 / forward_stage2), a parameter that never receives a
    gradient, a 0-dim parameter, and tensors whose sizes are no multiple of the flat buffers' 4-element padding"""

    def __init__(self, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.a = nn.Linear(7, 15)
        self.dead = nn.Linear(15, 15)
        self.b = nn.Linear(15, 3)
        self.s = nn.Parameter(torch.tensor(1.0))

    def forward(self, x):
        return self.forward_stage2(*self.forward_stage1(x))

    def forward_stage1(self, x):
        h = torch.tanh(self.a(x))
        return (h, h)

    def forward_stage2(self, h1, h2):
        return self.b(0.5 * (h1 + h2)) * self.s

    def stage1_parameters(self):
        return self.a.parameters()


class Toy3(Toy):
    """the same parameters cut into THREE stages through forward_stages()"""

    def forward_stages(self):
        s0 = lambda x: (self.a(x),)
        s1 = lambda h: (torch.tanh(h), torch.tanh(h))
        s2 = lambda h1, h2: (self.forward_stage2(h1, h2),)
        return [(s0, [self.a]), (s1, []), (s2, [self.b, _Holder(self.s)])]


class _Holder(nn.Module):
    def __init__(self, p):
        super().__init__()
        self.p = p


def _loss(o, t):
    return (o - t).pow(2).mean()


def _trainer(model, **kw):
    for k, v in HYPER.items():
        kw.setdefault(k, v)
    return FlatTrainer(model, _loss, use_graph=False, fused=False, **kw)


def _data(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(4, 7, generator=g), torch.randn(4, 3, generator=g)) for _ in range(n)]


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)


def _same(a, b, what=""):
    """two state dicts / nested containers: the same keys, tensors equal on bits, everything else equal"""
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what} differs"
    elif isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), f"{what}: keys {sorted(a)} vs {sorted(b) if isinstance(b, dict) else b}"
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    else:
        assert a == b, f"{what}: {a!r} vs {b!r}"


def _model_state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.fixture(scope="module")
def twin():
    """the uninterrupted run: 5 steps on one model; the trainer state and the model after steps 3 and 5"""
    data = _data(5)
    model = Toy()
    tr = _trainer(model)
    out = {"data": data}
    for i, (x, t) in enumerate(data, start=1):
        tr.step(x, t)
        if i in (3, 5):
            out[i] = (tr.state_dict(), _model_state(model))
    tr.close()
    return out


def test_state_dict_is_layout_independent_and_plain(twin):
    sd, _ = twin[3]
    assert sd["version"] == 1 and sd["steps"] == 3 and sd["micro_step"] == 0 and sd["accum_steps"] == 1 and sd["precision"] == "f32"
    assert (sd["lr"], sd["max_norm"], sd["betas"], sd["eps"], sd["weight_decay"]) == (1e-2, 0.5, (0.9, 0.999), 1e-9, 1e-2)
    assert sd["monitor"] is None and sd["fp8"] is None and sd["state_bits"].dtype == torch.int32 and sd["state_bits"].shape == (4,)
    shapes = {n: tuple(p.shape) for n, p in Toy().named_parameters()}
    assert set(sd["params"]) == {"a.weight", "a.bias", "b.weight", "b.bias", "s"}   # not the two `dead` tensors
    for n, ent in sd["params"].items():
        assert set(ent) == {"exp_avg", "exp_avg_sq"}
        for v in ent.values():
            assert v.device.type == "cpu" and tuple(v.shape) == shapes[n] and v.is_contiguous()
            assert v.untyped_storage().nbytes() == v.numel() * 4, f"{n}: the tensor drags a flat buffer along"
            assert bool(v.any()), f"{n}: three steps left a zero moment"


def test_round_trip_and_continuation(twin):
    sd3, model3 = twin[3]
    model = Toy(seed=11)
    assert not torch.equal(model.a.weight, model3["a.weight"])
    tr = _trainer(model, lr=0.5, max_norm=7.0)   # (both travel with the state)
    model.load_state_dict(model3)
    tr.load_state_dict(sd3)                      # before the first step: no flat buffer yet
    assert tr.used is None and tr._steps == 3 and tr.lr == 1e-2 and tr.max_norm == 0.5
    for x, t in twin["data"][3:]:
        tr.step(x, t)
    _same(tr.state_dict(), twin[5][0], "state after steps 4-5")
    _same(_model_state(model), twin[5][1], "model after steps 4-5")
    tr.close()


def test_load_after_the_first_step_gives_the_same_continuation(twin):
    sd3, model3 = twin[3]
    model = Toy(seed=12)
    tr = _trainer(model)
    tr.step(*_data(1, seed=99)[0])               # flat buffers exist, moments and parameters hold something else
    ptrs = [t.data_ptr() for t in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.state)]
    model.load_state_dict(model3)
    tr.load_state_dict(sd3)
    assert ptrs == [t.data_ptr() for t in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr.state)], "the load moved a buffer"
    _same(tr.state_dict(), sd3, "state right after the load")
    _same(_model_state(model), model3, "model right after the load")
    for x, t in twin["data"][3:]:
        tr.step(x, t)
    _same(tr.state_dict(), twin[5][0], "state after steps 4-5")
    _same(_model_state(model), twin[5][1], "model after steps 4-5")
    tr.close()


@pytest.mark.parametrize("src,dst", [("plain", "two"), ("two", "plain"), ("plain", "three"), ("three", "two")])
def test_any_layout_loads_any_other(src, dst):
    make = {"plain": lambda s: _trainer(Toy(s), overlap=False), "two": lambda s: _trainer(Toy(s), overlap=True),
            "three": lambda s: _trainer(Toy3(s), overlap=True)}
    data = _data(5, seed=6)
    a = make[src](0)
    for x, t in data[:3]:
        a.step(x, t)
    sd, msd = a.state_dict(), _model_state(a.model)
    for x, t in data[3:]:
        a.step(x, t)
    end = a.state_dict()
    b = make[dst](21)
    b.step(*data[0])
    assert len(b.buckets) == {"plain": 1, "two": 2, "three": 3}[dst] and len(a.buckets) == {"plain": 1, "two": 2, "three": 3}[src]
    name_of = {id(p): n for n, p in b.model.named_parameters()}
    if src != dst and {src, dst} != {"two", "three"}:
        assert [name_of[id(p)] for p in b.used] != [n for n in sd["params"]], "the two layouts order the parameters alike: nothing is tested"
    b.model.load_state_dict(msd)
    b.load_state_dict(sd)
    _same(b.state_dict(), sd, f"{src} -> {dst}")
    for i, p in enumerate(b.used):   # the flat buffers themselves, slice by slice
        for key, buf in (("exp_avg", b.exp_avg), ("exp_avg_sq", b.exp_avg_sq)):
            got = buf[b.offs[i]:b.offs[i] + p.numel()].view_as(p)
            assert torch.equal(got, sd["params"][name_of[id(p)]][key]), (name_of[id(p)], key)
    covered = torch.zeros(b.n, dtype=torch.bool)
    for i, p in enumerate(b.used):
        covered[b.offs[i]:b.offs[i] + p.numel()] = True
    assert not b.exp_avg[~covered].any() and not b.exp_avg_sq[~covered].any() and bool((~covered).any()), "padding must stay zero"
    for x, t in data[3:]:
        b.step(x, t)
    _same(b.state_dict(), end, f"{src} -> {dst}: two more steps")
    a.close()
    b.close()


def test_open_accumulation_cycle():
    data = _data(6, seed=7)
    a = _trainer(Toy(), accum_steps=3)
    for x, t in data[:2]:
        a.step(x, t)
    assert a.micro_step == 2
    sd, msd = a.state_dict(), _model_state(a.model)
    assert sd["micro_step"] == 2 and sd["accum_steps"] == 3 and sd["steps"] == 0
    assert all(set(e) == {"exp_avg", "exp_avg_sq", "acc"} for e in sd["params"].values())
    for x, t in data[2:]:
        a.step(x, t)
    want, want_sd = _model_state(a.model), a.state_dict()
    assert a._steps == 2 and "acc" not in want_sd["params"]["s"]
    for fresh in (True, False):
        b = _trainer(Toy(seed=31), accum_steps=3)
        if not fresh:
            b.step(*data[5])
            b.step(*data[4])
            b.step(*data[5])
            b.step(*data[4])     # (a cycle of its own is open: the load replaces it)
        b.model.load_state_dict(msd)
        b.load_state_dict(sd)
        assert b.micro_step == 2 and b._steps == 0
        if not fresh:
            _same(b.state_dict(), sd, "the open cycle right after the load")
        b.step(*data[2])
        assert b.micro_step == 0 and b._steps == 1
        for x, t in data[3:]:
            b.step(x, t)
        _same(_model_state(b.model), want, f"parameters after the resumed cycle (fresh={fresh})")
        _same(b.state_dict(), want_sd, f"state after the resumed cycle (fresh={fresh})")
        b.close()
    c = _trainer(Toy(), accum_steps=2)
    with pytest.raises(RuntimeError, match="accum_steps=3.*accum_steps=2"):
        c.load_state_dict(sd)
    assert c.micro_step == 0 and c._pending is None
    c.load_state_dict(want_sd)   # between cycles another accum_steps is fine
    assert c.accum_steps == 2 and c._steps == 2
    c.close()
    a.close()


def test_monitor_block_travels():
    data = _data(4, seed=8)
    a = _trainer(Toy(), monitor=True)
    for x, t in data[:2]:
        a.step(x, t)
    bad = data[2][0].clone()
    bad[0, 0] = float("inf")
    a.step(bad, data[2][1])
    sd, msd = a.state_dict(), _model_state(a.model)
    assert sd["monitor"].dtype == torch.float64 and sd["monitor"].shape == (9,) and sd["steps"] == 2
    a.step(*data[3])
    want = a.stats()
    assert want["steps"] == 3 and want["skipped"] == 1
    b = _trainer(Toy(seed=41), monitor=True)
    b.model.load_state_dict(msd)
    b.load_state_dict(sd)
    b.step(*data[3])
    assert b.stats() == want
    _same(b.state_dict(), a.state_dict(), "monitored run")
    a.close()
    b.close()


def test_training_state_file(twin, tmp_path):
    data = twin["data"]
    model = Toy()
    tr = _trainer(model)
    for x, t in data[:3]:
        tr.step(x, t)
    path = str(tmp_path / "state.pth")
    stats = {"norm_mean": 0.125, "steps": 3}
    assert checkpoint.save_training_state(tr, path, schedule_stats=stats) == len(model.state_dict())
    tr.close()
    other = Toy(seed=51)
    assert checkpoint.load_reference_checkpoint(other, path) == len(model.state_dict())   # the model part is a reference checkpoint
    _same(_model_state(other), twin[3][1], "model part")
    fresh = Toy(seed=52)
    tr2 = _trainer(fresh)
    assert checkpoint.load_training_state(tr2, path) == stats
    for x, t in data[3:]:
        tr2.step(x, t)
    _same(tr2.state_dict(), twin[5][0], "state after the file round trip")
    _same(_model_state(fresh), twin[5][1], "model after the file round trip")
    tr2.close()
    plain = str(tmp_path / "best.pth")
    checkpoint.save_reference_checkpoint(fresh, plain)
    with pytest.raises(RuntimeError, match="save_training_state"):
        checkpoint.load_training_state(_trainer(Toy()), plain)


def test_torch_adamw_interop(twin):
    sd3, model3 = twin[3]
    model = Toy(seed=61)
    tr = _trainer(model, max_norm=0.0)
    tr.step(*twin["data"][0])
    model.load_state_dict(model3)
    tr.load_state_dict(sd3)
    tr.max_norm = 0.0
    opt_sd = checkpoint.to_torch_adamw_state(tr)
    params = list(model.parameters())
    assert sorted(opt_sd["state"]) == [i for i, p in enumerate(params) if any(p is q for q in tr.used)] and len(opt_sd["state"]) == 5
    assert all(float(s["step"]) == 3.0 for s in opt_sd["state"].values())
    g = opt_sd["param_groups"][0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]) == (1e-2, (0.9, 0.999), 1e-9, 1e-2)
    # the identity, on bits
    before = tr.state_dict()
    checkpoint.from_torch_adamw_state(tr, opt_sd)
    _same(tr.state_dict(), before, "from_torch_adamw_state(to_torch_adamw_state(tr))")
    # one torch step against one step of the trainer's own statement of the rule, on the same gradient
    ref = Toy(seed=62)
    ref.load_state_dict(model3)
    opt = torch.optim.AdamW(ref.parameters(), lr=123.0, eps=1e-3)
    opt.load_state_dict(opt_sd)
    x, t = twin["data"][3]
    _loss(ref(x), t).backward()
    assert ref.dead.weight.grad is None
    opt.step()
    tr.step(x, t)
    for (k, a), (_, b) in zip(model.named_parameters(), ref.named_parameters()):
        assert_close(a, b, 2e-5, k, atol=1e-6)   # tests/test_trainer_gpu.py's bar for the trainer against torch.optim.AdamW
    # and back: the torch optimiser's state after its step continues here (fresh trainer: the state waits for the layout)
    back = Toy(seed=63)
    back.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()})
    tr2 = _trainer(back, max_norm=0.0, lr=5.0)
    checkpoint.from_torch_adamw_state(tr2, opt.state_dict())
    assert tr2._steps == 4 and tr2.lr == 1e-2
    x, t = twin["data"][4]
    tr2.step(x, t)
    tr.step(x, t)
    for (k, a), (_, b) in zip(back.named_parameters(), model.named_parameters()):
        assert_close(a, b, 2e-5, k, atol=1e-6)
    with pytest.raises(RuntimeError, match="betas"):
        bad = opt.state_dict()
        bad["param_groups"][0]["betas"] = (0.8, 0.999)
        checkpoint.from_torch_adamw_state(tr, bad)
    tr.close()
    tr2.close()


def test_errors_name_the_offender(twin):
    sd3, model3 = twin[3]

    def ready(**kw):
        tr = _trainer(Toy(), **kw)
        tr.step(*twin["data"][0])
        return tr

    def edited(fn):
        sd = dict(sd3)
        sd["params"] = {n: dict(e) for n, e in sd3["params"].items()}
        fn(sd)
        return sd
    tr = ready()
    before = tr.state_dict()
    with pytest.raises(RuntimeError, match=r"b\.bias"):
        tr.load_state_dict(edited(lambda sd: sd["params"].pop("b.bias")))
    with pytest.raises(RuntimeError, match=r"dead\.weight"):
        tr.load_state_dict(edited(lambda sd: sd["params"].update({"dead.weight": {"exp_avg": torch.zeros(15, 15), "exp_avg_sq": torch.zeros(15, 15)}})))
    with pytest.raises(RuntimeError, match=r"nobody\.weight"):
        tr.load_state_dict(edited(lambda sd: sd["params"].update({"nobody.weight": sd["params"]["a.weight"]})))
    with pytest.raises(RuntimeError, match=r"exp_avg_sq of a\.weight.*\(15, 8\)"):
        tr.load_state_dict(edited(lambda sd: sd["params"]["a.weight"].update(exp_avg_sq=torch.zeros(15, 8))))
    with pytest.raises(RuntimeError, match="version"):
        tr.load_state_dict(edited(lambda sd: sd.update(version=0)))
    _same(tr.state_dict(), before, "a refused load wrote something")
    tr.close()
    # a fresh trainer refuses a missing name when its layout is made
    tr = _trainer(Toy())
    tr.load_state_dict(edited(lambda sd: sd["params"].pop("b.bias")))
    with pytest.raises(RuntimeError, match=r"b\.bias"):
        tr.step(*twin["data"][0])
    tr.close()
    # hyper-parameters: refused by name, accepted with strict=False (the trainer keeps its own)
    tr = ready(betas=(0.8, 0.999))
    with pytest.raises(RuntimeError, match=r"betas.*0\.9.*0\.8"):
        tr.load_state_dict(sd3)
    tr.load_state_dict(sd3, strict=False)
    assert tr.betas == (0.8, 0.999) and tr._steps == 3
    got = tr.state_dict()
    _same(got["params"], sd3["params"], "moments under strict=False")
    tr.close()
    for kw, word in ((dict(eps=1e-8), "eps"), (dict(weight_decay=0.0), "weight_decay")):
        tr = ready(**kw)
        with pytest.raises(RuntimeError, match=word):
            tr.load_state_dict(sd3)
        tr.close()
    # precision
    tr = ready()
    ops.set_mfma_precision("bf16")
    try:
        with pytest.raises(RuntimeError, match=r"precision 'f32'.*'bf16'"):
            tr.load_state_dict(sd3)
        with pytest.raises(RuntimeError, match="precision"):
            tr.load_state_dict(sd3, strict=False)   # strict=False relaxes the hyper-parameter check only
    finally:
        ops.set_mfma_precision("f32")
    tr.load_state_dict(sd3)
    tr.close()
    with pytest.raises(RuntimeError, match="flat buffers do not exist"):
        _trainer(Toy()).state_dict()


def test_defaults_allocate_nothing():
    tr = _trainer(Toy())
    tr.step(*_data(1)[0])
    assert tr._pending is None and tr._pending_quant is None and tr.acc is None and tr._stats is None
    snap = tr.snapshot()          # the CPU form of snapshot(): copies made at once
    tr.step(*_data(1)[0])
    sd = snap.state_dict()
    assert sd["steps"] == 1 and set(sd["parameters"]) == set(sd["params"])
    assert tr.state_dict()["steps"] == 2
    tr.close()
