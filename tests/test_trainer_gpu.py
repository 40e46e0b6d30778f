"""FlatTrainer on the GPU: the fused clip + AdamW kernels against torch.nn.utils.clip_grad_norm_ +
torch.optim.AdamW (the reference's recipe, train.py:140, train_untils.py:35-42), eager and hipGraph replay."""
import copy
import pytest
import torch

from adnm_hip import recipe
from adnm_hip.trainer import FlatTrainer
from util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"


def small_model():
    from models.ADNMUNet import create_block
    torch.manual_seed(0)
    m = create_block(32, 16, headdim=4, norm_epsilon=1e-6)
    recipe.fill_parameters(m)
    return m.to(DEV)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("max_norm", [0.0, 0.05])
def test_fused_step_matches_torch(use_graph, max_norm):
    ref = small_model()
    mine = copy.deepcopy(ref)
    x, tgt = recipe.tensor("tr.x", (2, 64, 32)).to(DEV), recipe.tensor("tr.t", (2, 64, 16)).to(DEV)
    loss_fn = lambda o, t: ((o - t) ** 2).mean()
    opt = torch.optim.AdamW(ref.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2)
    tr = FlatTrainer(mine, loss_fn, lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=max_norm, use_graph=use_graph)
    for step in range(4):
        loss_ref = loss_fn(ref(x), tgt)
        loss_ref.backward()
        if max_norm > 0:
            norm_ref = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm)
        opt.step()
        opt.zero_grad(set_to_none=True)
        loss = tr.step(x, tgt)
        assert abs(float(loss) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref)) + 1e-7
        if max_norm > 0:
            assert abs(float(tr.grad_norm()) - float(norm_ref)) <= 1e-4 * float(norm_ref)
    for (k, a), (_, b) in zip(mine.named_parameters(), ref.named_parameters()):
        assert_close(a, b, 2e-5, k, atol=1e-6)
    # parameters that never receive a gradient are untouched (no decay), as torch.optim.AdamW leaves them
    unused = [k for k, p in mine.named_parameters() if all(p is not q for q in tr.used)]
    assert "alpha1" in unused and "act.beta" in unused


@pytest.mark.parametrize("use_graph,stages", [(False, False), (True, False), (False, True), (True, True)])
def test_whole_model_step_vs_reference_fixture(use_graph, stages):
    """FlatTrainer (flat buffers, channels-last conv weights, in-place gradient destinations, hipGraph replay, fused
    clip + AdamW) on the whole ADNM-UNet: loss, pre-clip gradient norm and every parameter after one step against the values the
    reference produced with clip_grad_norm_(0.025) + torch.optim.AdamW (tests/golden, train.py:140, train_untils.py:35-42)."""
    from models.ADNMUNet import create_ADNMUNet
    from models.loss import enRainfallLoss
    from util import load_npz
    z = load_npz("visionmamba_64_b2")
    model = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(model)
    model = model.to(DEV).train()
    frames = recipe.radar_batch(2, 25, 64, name="radar64").to(DEV)
    x, tgt = frames[:, :5], frames[:, 5:]
    # stages=True: the two-stage backward (encoder | decoder + refiner, two graphs) that multi-GPU runs use to overlap the gradient
    # all-reduce with the encoder's backward — same numbers required
    tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                     use_graph=use_graph, stages=stages)
    assert tr.staged == stages
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    loss = tr.step(x, tgt)
    assert abs(float(loss) - float(z["loss"])) <= 1e-4 * abs(float(z["loss"]))
    assert abs(float(tr.grad_norm()) - float(z["clip_pre_norm"])) <= 1e-3 * float(z["clip_pre_norm"])
    if stages:   # five stages (refiner | decoder blocks | e2ds + fusion | encoder4-6 | encoder1-3): five graphs, five buckets
        assert len(tr.stage_defs) == 5 and len(tr.buckets) == 5 and len(tr.graphs) == (4 if use_graph else 0)
        assert 0 < tr.n_late < tr.n and all(len(g) > 20 for g in tr.groups)
    names, ref_sums, gn = [str(n) for n in z["names"]], z["param_sum_after_step"].numpy(), z["grad_norms"].numpy()
    named = dict(model.named_parameters())
    for i, k in enumerate(names):
        p = named[k]
        s = float(p.double().sum())
        assert abs(s - ref_sums[i]) <= 2.5e-3 * p.numel() ** 0.5 + 1e-5 * abs(ref_sums[i]) + 1e-6, k
        if gn[i] < 0:   # the reference leaves these without a gradient: neither updated nor decayed
            assert torch.equal(p, before[k]), k
    # state_dict still has the reference's logical shapes (conv weights are channels-last views of the flat buffer)
    assert model.state_dict()["refiner.out_proj.conv.0.conv.weight"].shape == (64, 32, 3, 3)


def test_benchmarked_workload_step_vs_reference_fixture():
    """The exact workload bench.py times (B=4, 128x128, 5->20, recipe batch "bench", hipGraph replay, fused clip + AdamW): loss,
    pre-clip norm and the UPDATE of every parameter (p_after - p_before; element-wise for the 360 scalar mixes) against what the
    reference produced for the same batch (fixture visionmamba_128_b4, oracle/make_golden.py)."""
    from models.ADNMUNet import create_ADNMUNet
    from models.loss import enRainfallLoss
    from util import load_npz, check_update_deltas
    z = load_npz("visionmamba_128_b4")
    model = create_ADNMUNet(5, 20, 6, img_size=128)
    recipe.fill_parameters(model)
    model = model.to(DEV).train()
    frames = recipe.radar_batch(4, 25, 128, name="bench").to(DEV)
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                     use_graph=True)
    before = [p.detach().double().clone() for p in model.parameters()]
    loss = tr.step(x, tgt)
    assert abs(float(loss) - float(z["loss"])) <= 1e-4 * abs(float(z["loss"]))
    assert abs(float(tr.grad_norm()) - float(z["clip_pre_norm"])) <= 1e-3 * float(z["clip_pre_norm"])
    names = [str(n) for n in z["names"]]
    assert names == [k for k, _ in model.named_parameters()]
    check_update_deltas(z, names, [p.detach().double() - b for p, b in zip(model.parameters(), before)])


def test_benchmarked_workload_bf16_with_shadow():
    """bench.py's configuration as it is timed: B=4, 128x128, recipe batch "bench", bf16 matrix-core operands, the bf16 weight shadow,
    hipGraph replay.  First step against the reference's fp32 fixture (visionmamba_128_b4) within bf16 bars; 20 steps train (finite
    parameters, the loss goes down) and leave the shadow bit for bit bf16(p)."""
    from models.ADNMUNet import create_ADNMUNet
    from models.loss import enRainfallLoss
    from adnm_hip import ops
    from util import load_npz
    z = load_npz("visionmamba_128_b4")
    frames = recipe.radar_batch(4, 25, 128, name="bench").to(DEV)
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    ops.set_mfma_precision("bf16")
    try:
        model = create_ADNMUNet(5, 20, 6, img_size=128)
        recipe.fill_parameters(model)
        model = model.to(DEV).train()
        tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                         use_graph=True)
        try:
            losses = [float(tr.step(x, tgt))]
            norm = float(tr.grad_norm())
            for _ in range(19):
                losses.append(float(tr.step(x, tgt)))
            torch.cuda.synchronize()
            assert tr.shadow_mode == 1 and tr.graph is not None
            dl = abs(losses[0] - float(z["loss"])) / abs(float(z["loss"]))
            dn = abs(norm - float(z["clip_pre_norm"])) / float(z["clip_pre_norm"])
            print(f"bf16 bench workload: first-step loss {losses[0]:.6f} ({dl:.2e} from the fp32 reference), pre-clip norm {norm:.6f} ({dn:.2e}); "
                  f"loss after 20 steps {losses[-1]:.6f}")
            assert dl <= 0.02, f"first-step loss {losses[0]} vs reference {float(z['loss'])}"
            assert dn <= 0.05, f"first-step pre-clip norm {norm} vs reference {float(z['clip_pre_norm'])}"
            bad = [k for k, p in model.named_parameters() if not bool(torch.isfinite(p).all())]
            assert not bad, f"non-finite parameters after 20 steps: {bad[:5]}"
            assert losses[-1] < losses[0], losses
            assert torch.equal(tr.shadow, tr.flat_p.to(torch.bfloat16)), "the shadow is bf16(p) after every step"
        finally:
            tr.close()
    finally:
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()


def test_deferred_folds_are_neutral_and_deterministic():
    """Batching the second-stage fold launches of the parameter gradients and grouping the weight-gradient launches (ops.FOLDS /
    adnm_foldq_* / adnm_leafq_*) must not change the step beyond fp32 summation order — a queued weight gradient splits its reduction
    into fewer slices than one launched alone, the fold arithmetic itself is the same — including Block.beta1/beta2, which receive two
    contributions; and the deferred step is deterministic: two runs agree bit for bit (no atomics anywhere)."""
    from models.ADNMUNet import create_ADNMUNet
    from models.loss import enRainfallLoss
    frames = recipe.radar_batch(1, 25, 64, name="defer").to(DEV)
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    flats = []
    for defer in (False, True, True):
        model = create_ADNMUNet(5, 20, 6, img_size=64)
        recipe.fill_parameters(model)
        model = model.to(DEV).train()
        tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), max_norm=0.025, use_graph=False, defer_folds=defer)
        tr.prepare(x, tgt)
        from adnm_hip import lib
        lib.query("adnm_prof_enable", 1)
        tr._run_eager(x, tgt)
        torch.cuda.synchronize()
        lib.query("adnm_prof_enable", 0)
        import ctypes
        buf = ctypes.create_string_buffer(1 << 20)
        lib.query("adnm_prof_collect", buf, len(buf))
        nfold = sum(int(l.split("\t")[1]) for l in buf.value.decode().splitlines() if "fold" in l.split("\t")[0])
        flats.append((tr.flat_g.clone(), nfold))
        tr.close()
        del tr
    assert torch.equal(flats[1][0], flats[2][0]), "the deferred step is not deterministic"
    a, b = flats[0][0].double(), flats[1][0].double()
    assert float((a - b).norm()) <= 1e-6 * float(a.norm()), float((a - b).norm() / a.norm())
    assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max())
    assert flats[1][1] < 0.5 * flats[0][1], (flats[0][1], flats[1][1])


def test_bf16_wire_casts_on_the_real_bucket_boundaries():
    """The bf16 wire format of the gradient all-reduce (reduce_dtype="bf16"): the HIP cast kernels need 16-byte aligned ranges on both
    sides, so every stage boundary of the staged layout must fall on a multiple of 8 elements — checked on the benchmarked model's
    real five buckets, with the round trip through the wire buffer (a single process cannot run the collective itself)."""
    from models.ADNMUNet import create_ADNMUNet
    from models.loss import enRainfallLoss
    model = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(model)
    model = model.to(DEV).train()
    frames = recipe.radar_batch(1, 25, 64, name="wire").to(DEV)
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), max_norm=0.025, use_graph=False, overlap=True, reduce_dtype="bf16")
    tr.prepare(x, tgt)
    tr._run_eager(x, tgt)
    assert len(tr.buckets) == 5 and all(lo % 8 == 0 for lo, _ in tr.buckets)
    comm = torch.zeros(tr.n, dtype=torch.bfloat16, device=DEV)   # (zeros: the alignment gaps between buckets belong to no bucket)
    back = torch.empty_like(tr.flat_g)
    for lo, hi in tr.buckets:
        tr._cast(tr.flat_g[lo:hi], comm[lo:hi])
        tr._cast(comm[lo:hi], back[lo:hi], 0.5)
    torch.cuda.synchronize()
    for lo, hi in tr.buckets:
        assert torch.equal(comm[lo:hi], tr.flat_g[lo:hi].to(torch.bfloat16))
        assert torch.equal(back[lo:hi], comm[lo:hi].float() * 0.5)


def test_bf16_shadow_weights_are_bitwise_neutral(monkeypatch):
    """The bf16 configuration reads its GEMM weights from the bf16 shadow the optimiser pass writes (and the mixer prep's bf16 copies):
    rounding the fp32 weight on the way into the MFMA or reading its pre-rounded twin is the same arithmetic — parameters and gradients
    after several steps must agree bit for bit with ADNM_NARROW_WEIGHTS=0."""
    from models.ADNMUNet import create_ADNMUNet
    from models.loss import enRainfallLoss
    from adnm_hip import ops
    frames = recipe.radar_batch(2, 25, 64, name="shadow").to(DEV)
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    flats = []
    ops.set_mfma_precision("bf16")
    try:
        for narrow in ("0", "1"):
            monkeypatch.setenv("ADNM_NARROW_WEIGHTS", narrow)
            model = create_ADNMUNet(5, 20, 6, img_size=64)
            recipe.fill_parameters(model)
            model = model.to(DEV).train()
            tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, max_norm=0.025, use_graph=True)
            for _ in range(4):
                tr.step(x, tgt)
            torch.cuda.synchronize()
            assert (getattr(tr, "shadow_mode", 0) == 1) == (narrow == "1")
            if narrow == "1":
                assert torch.equal(tr.shadow, tr.flat_p.to(torch.bfloat16)), "the shadow is bf16(p) after every step"
            flats.append((tr.flat_p.clone(), tr.flat_g.clone()))
            tr.close()
            del tr
    finally:
        ops.set_mfma_precision("f32")
    assert torch.equal(flats[0][1], flats[1][1]), "gradients differ with the shadow weights"
    assert torch.equal(flats[0][0], flats[1][0]), "parameters differ with the shadow weights"


def test_tail_graph_follows_host_schedules():
    """The staged trainer (the multi-GPU form) replays its optimiser as a captured TAIL graph whose learning rate and clip threshold live in
    device memory: changing tr.lr / tr.max_norm between steps (train.py's warm-up + cosine schedule, its adaptive clip threshold) must give
    bit for bit what the eagerly launched optimiser gives."""
    from models.ADNMUNet import create_ADNMUNet
    from models.loss import enRainfallLoss
    frames = recipe.radar_batch(2, 25, 64, name="tail").to(DEV)
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    flats = []
    for use_graph in (False, True):
        model = create_ADNMUNet(5, 20, 6, img_size=64)
        recipe.fill_parameters(model)
        model = model.to(DEV).train()
        tr = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, max_norm=0.025, use_graph=use_graph, overlap=True)
        for k in range(5):
            tr.lr, tr.max_norm = 1e-3 * (1.0 - 0.15 * k), 0.025 * (1.0 + 0.5 * k)
            tr.step(x, tgt)
        torch.cuda.synchronize()
        assert tr.staged and (getattr(tr, "tail", None) is not None) == use_graph
        flats.append((tr.flat_p.clone(), tr.exp_avg.clone()))
        tr.close()
        del tr
    assert torch.equal(flats[0][1], flats[1][1]) and torch.equal(flats[0][0], flats[1][0])


@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_failed_tail_capture_leaves_the_trainer_as_before_prepare(prec, monkeypatch):
    """prepare() of the staged trainer warms its tail up with a real optimiser pass and puts parameters, moments and step counter back
    afterwards.  An ordinary Python exception inside the tail capture (here: _tail_body raises at the end of its second call) must not
    skip that: the trainer holds what a twin built from the same seed holds after a successful prepare() — which is what it held before:
    the filled parameters, zero moments, a zero step counter —, no graph, no pin on the fp8 table, and after close() the model trains
    under a fresh trainer."""
    from models.ADNMUNet import create_ADNMUNet
    from models.loss import enRainfallLoss
    from adnm_hip import ops
    frames = recipe.radar_batch(1, 25, 64, name="tailfail").to(DEV)
    x, tgt = frames[:, :5].contiguous(), frames[:, 5:].contiguous()
    names = ("flat_p", "exp_avg", "exp_avg_sq", "state", "flat_g", "shadow")

    def build():
        model = create_ADNMUNet(5, 20, 6, img_size=64)
        recipe.fill_parameters(model)
        model = model.to(DEV).train()
        return model, FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, max_norm=0.025, use_graph=True, overlap=True)

    ops.set_mfma_precision(prec)
    try:
        model, twin = build()
        filled = [p.detach().clone() for p in model.parameters()]
        twin.prepare(x, tgt)
        torch.cuda.synchronize()
        assert twin.tail is not None and (twin.shadow_mode == 2) == (prec == "fp8")
        assert all(torch.equal(p, q) for p, q in zip(model.parameters(), filled)), "prepare() moved the parameters"
        assert not twin.exp_avg.any() and not twin.exp_avg_sq.any() and not twin.state.any(), "prepare() moved the optimiser state"
        want = {k: getattr(twin, k).clone() for k in names}
        want_q = ops.QUANT.snapshot(x.device)   # (record table, calibration state): clones
        twin.close()
        del twin, model

        model, tr = build()
        pins0 = ops.QUANT.pins(x.device)
        real, calls = tr._tail_body, [0]

        def tail_body():
            calls[0] += 1
            real()
            if calls[0] == 2:   # the call inside the capture
                raise ValueError("boom")
        monkeypatch.setattr(tr, "_tail_body", tail_body)
        with pytest.raises(ValueError):
            tr.prepare(x, tgt)
        torch.cuda.synchronize()
        assert calls[0] == 2
        assert tr.tail is None and tr.graph is None and tr.graphs == [] and tr.sx is None and tr.st is None
        assert ops.QUANT.pins(x.device) == pins0
        for k in names:
            assert torch.equal(getattr(tr, k), want[k]), f"{k} differs from its value before prepare()"
        assert all(torch.equal(a, b) for a, b in zip(ops.QUANT.snapshot(x.device), want_q)), "the fp8 table differs from its value before prepare()"
        tr.close()
        assert ops.QUANT.pins(x.device) == pins0

        tr2 = FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, max_norm=0.025, use_graph=True, overlap=True)
        tr2.prepare(x, tgt)
        loss = tr2.step(x, tgt)
        torch.cuda.synchronize()
        assert tr2.tail is not None and bool(torch.isfinite(loss))
        assert tr2.exp_avg.any() and not torch.equal(tr2.flat_p, want["flat_p"]), "the step ran no optimiser pass"
        tr2.close()
    finally:
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()


def test_graphed_forward_failed_capture_gives_the_pin_back():
    """A model forward that raises inside GraphedForward's capture (fp8: the pin on the quantisation table is already taken) leaves the
    pin count where it was and the model in its mode; close() is idempotent, and the same object captures once the forward works."""
    from models.ADNMUNet import create_ADNMUNet
    from adnm_hip import ops
    from adnm_hip.evaluator import GraphedForward

    class FailsOnThird(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner, self.calls = inner, 0

        def forward(self, x):
            self.calls += 1
            out = self.inner(x)
            if self.calls == 3:   # two warm-up calls, then the one inside the capture
                raise ValueError("boom")
            return out

    inner = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(inner)
    model = FailsOnThird(inner.to(DEV)).train()
    x = recipe.radar_batch(1, 25, 64, name="evalfail").to(DEV)[:, :5].contiguous()
    try:
        with torch.no_grad():
            model.eval()
            ops.fp8_calibrate(x.device, lambda: inner(x))   # every call site's record; leaves the precision at fp8
            model.train()
        pins0 = ops.QUANT.pins(x.device)
        fwd = GraphedForward(model)
        with pytest.raises(ValueError):
            fwd(x)
        torch.cuda.synchronize()
        assert model.calls == 3 and model.training
        assert ops.QUANT.pins(x.device) == pins0
        fwd.close()
        fwd.close()
        assert ops.QUANT.pins(x.device) == pins0
        out = fwd(x)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and ops.QUANT.pins(x.device) == pins0 + 1
        fwd.close()
        fwd.close()
        assert ops.QUANT.pins(x.device) == pins0
    finally:
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()
