"""The resident data feed on the GPU: adnm_batch_fetch against torch's own indexing, bit for bit, on both of its paths
(16-byte pieces, single floats) and with indices it must not follow; the store ResidentDataset builds against dataio.ingest; and
FlatTrainer.step_from / Validator.step_from against step(x, tgt) on the same batches, bitwise."""
import pytest
import torch

from adnm_hip import dataio, lib, ops, recipe
from adnm_hip.dataio import ResidentDataset

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, T, T_IN = 7, 5, 2


def _stream():
    return torch.cuda.current_stream().cuda_stream


_stores = {}


def _store(S, n=N, t=T):
    """(n, t, S, S) random fp32 on the device, made once per shape and never written"""
    key = (n, t, S)
    if key not in _stores:
        _stores[key] = recipe.tensor(f"feed.store.{n}.{t}.{S}", (n, t, S, S)).to(DEV)
    return _stores[key]


def _guarded(numel, lead):
    """-> (the whole allocation, NaN everywhere; the `numel` floats that start `lead` floats into it)"""
    whole = torch.full((lead + numel + 16,), float("nan"), device=DEV)
    return whole, whole[lead:lead + numel]


def _fetch_and_check(store, order, pos, B, t_in, lead_x=16, lead_t=16, bad=()):
    n, t, S, _ = store.shape
    hw = S * S
    wx, x = _guarded(B * t_in * hw, lead_x)
    wt, tgt = _guarded(B * (t - t_in) * hw, lead_t)
    assert x.data_ptr() % 16 == (4 * lead_x) % 16
    lib.call("adnm_batch_fetch", store.data_ptr(), n, t, hw, order.data_ptr(), order.numel(), pos, x.data_ptr(), tgt.data_ptr(), B, t_in, _stream())
    torch.cuda.synchronize()
    idx = order[pos:pos + B].long()
    x, tgt = x.view(B, t_in, S, S), tgt.view(B, t - t_in, S, S)
    for b in range(B):
        s = int(idx[b])
        if s in bad:
            assert bool(torch.isnan(x[b]).all()) and bool(torch.isnan(tgt[b]).all()), f"sample {b} (index {s}) must be all NaN"
        else:
            assert torch.equal(x[b], store[s, :t_in]) and torch.equal(tgt[b], store[s, t_in:]), f"sample {b} (index {s}) is not an exact copy"
    for whole, lead, numel in ((wx, lead_x, x.numel()), (wt, lead_t, tgt.numel())):
        assert bool(torch.isnan(whole[:lead]).all()) and bool(torch.isnan(whole[lead + numel:]).all()), "the fetch wrote outside its destination"
    return x, tgt


@pytest.mark.parametrize("pos", [0, 2])
@pytest.mark.parametrize("S", [8, 9, 16])
def test_fetch_is_an_exact_copy(S, pos):
    """S = 9: hw = 81, the sample stride 405 and the split point 162 are no multiples of 4 (single floats); S = 8, 16: 16-byte pieces"""
    store = _store(S)
    order = torch.tensor([3, 0, 3, N - 1, 3], dtype=torch.int32, device=DEV)   # pos 0: 3, 0, 3; pos 2: 3, N - 1, 3
    x, tgt = _fetch_and_check(store, order, pos, 3, T_IN)
    idx = order[pos:pos + 3].long()
    assert torch.equal(x, store[idx][:, :T_IN]) and torch.equal(tgt, store[idx][:, T_IN:])


@pytest.mark.parametrize("lead_x,lead_t", [(17, 16), (16, 18), (19, 19)])
def test_fetch_into_a_slice_that_is_only_4_byte_aligned_is_served(lead_x, lead_t):
    """include/adnm_hip.h: such a call is served, not refused (the entry point falls back to single floats)"""
    order = torch.tensor([6, 1, 1], dtype=torch.int32, device=DEV)
    _fetch_and_check(_store(8), order, 0, 3, T_IN, lead_x=lead_x, lead_t=lead_t)


@pytest.mark.parametrize("S,B", [(64, 3), (128, 256), (127, 256)])
def test_fetch_over_more_than_one_workgroup_per_sample(S, B):
    """S = 64: 5 workgroups a sample.  B = 256: the grid is capped at 2048 / 256 = 8 workgroups a sample, each of which makes several
    trips with a ragged last one (16-byte pieces at S = 128, single floats at S = 127)"""
    store = _store(S, n=4)
    order = (torch.arange(B + 3, dtype=torch.int32) * 7 % 4).to(DEV)
    _fetch_and_check(store, order, 3, B, T_IN)


@pytest.mark.parametrize("S", [8, 9])
def test_an_index_outside_the_store_gives_nans_and_is_not_followed(S):
    order = torch.tensor([1, N, 0, -1, N - 1, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV)
    _fetch_and_check(_store(S), order, 0, order.numel(), T_IN, bad=(N, -1, 2 ** 31 - 1, -2 ** 31))
    torch.cuda.synchronize()   # no error from the launch


def test_from_bytes_is_ingest_per_sample_and_from_frames_keeps_its_input():
    n, t, H0, W0, S = 5, 4, 40, 56, 16
    g = torch.Generator().manual_seed(11)
    raw = torch.randint(0, 71, (n, t, H0, W0), dtype=torch.uint8, generator=g)
    feed = ResidentDataset.from_bytes(raw, S, in_frames=1, batch=2, device=DEV, shuffle=False, chunk=2)   # chunks of 2, 2, 1 samples
    assert tuple(feed.store.shape) == (n, t, S, S) and len(feed) == 2 and feed.store_bytes == n * t * S * S * 4
    for i in range(n):
        assert torch.equal(feed.store[i], dataio.ingest(raw[i:i + 1].to(DEV), S)[0, :, 0]), f"sample {i}"
    same = ResidentDataset.from_bytes(raw.numpy(), S, in_frames=1, batch=2, device=DEV, shuffle=False, chunk=64)
    assert torch.equal(same.store, feed.store)
    frames = recipe.tensor("feed.frames", (n, t, 12, 12))
    kept = ResidentDataset.from_frames(frames, in_frames=3, batch=2, device=DEV, shuffle=False)
    assert torch.equal(kept.store.cpu(), frames)
    # the feed itself: sequential order, shapes with the channel axis, the end of an epoch
    with pytest.raises(RuntimeError, match="no epoch yet"):
        kept.fetch()
    kept.begin_epoch()
    x, tgt = kept.fetch()
    assert tuple(x.shape) == (2, 3, 1, 12, 12) and tuple(tgt.shape) == (2, 1, 1, 12, 12)
    assert torch.equal(x[:, :, 0].cpu(), frames[0:2, :3]) and torch.equal(tgt[:, :, 0].cpu(), frames[0:2, 3:])
    x, tgt = kept.fetch()
    assert torch.equal(x[:, :, 0].cpu(), frames[2:4, :3])
    with pytest.raises(IndexError):
        kept.fetch()
    with pytest.raises(RuntimeError, match="fetch_into"):
        kept.fetch_into(torch.empty(2, 3, 1, 12, 13, device=DEV), tgt)


def test_a_restored_feed_goes_on_with_the_same_batches():
    frames = recipe.tensor("feed.resume", (9, 3, 4, 4))
    a = ResidentDataset.from_frames(frames, 1, 2, DEV, generator=torch.Generator().manual_seed(21))
    a.begin_epoch()
    a.fetch()
    sd = a.state_dict()
    b = ResidentDataset.from_frames(frames, 1, 2, DEV, generator=torch.Generator().manual_seed(5))
    b.load_state_dict(sd)
    for _ in range(len(a) - 1):
        (xa, ta), (xb, tb) = a.fetch(), b.fetch()
        assert torch.equal(xa, xb) and torch.equal(ta, tb)
    a.begin_epoch(), b.begin_epoch()
    assert torch.equal(a.fetch()[0], b.fetch()[0])


# ------------------------------------------------------------------------------------------------ the consumers
def _model():
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(m)
    return m.to(DEV).train()


_samples = {}


def _feed(batch=2):
    if "f" not in _samples:
        _samples["f"] = recipe.radar_batch(6, 25, 64, name="feed.e2e")[:, :, 0].contiguous()
    return ResidentDataset.from_frames(_samples["f"], 5, batch, DEV, shuffle=True, generator=torch.Generator().manual_seed(3))


def _trainer(accum):
    from adnm_hip.trainer import FlatTrainer
    from models.loss import enRainfallLoss
    return FlatTrainer(_model(), enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                       use_graph=True, accum_steps=accum)


@pytest.mark.parametrize("accum,calls", [(1, 3), (2, 2)])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_step_from_is_step_on_the_same_batches(prec, accum, calls):
    ops.set_mfma_precision(prec)
    ops.QUANT.reset()
    a = b = None
    try:
        feed, twin = _feed(), _feed()
        feed.begin_epoch(), twin.begin_epoch()
        assert len(feed) == 3
        a, b = _trainer(accum), _trainer(accum)
        la, lb, ptrs = [], [], []
        for _ in range(calls):
            la.append(a.step_from(feed).detach().clone())
            ptrs.append((a.sx.data_ptr(), a.st.data_ptr()))
        for _ in range(calls):
            lb.append(b.step(*twin.fetch()).detach().clone())
        torch.cuda.synchronize()
        assert len(set(ptrs)) == 1, "step_from moved the static buffers"
        assert a.micro_step == b.micro_step == 0
        for i, (x, y) in enumerate(zip(la, lb)):
            assert bool(torch.isfinite(x)) and torch.equal(x.view(torch.int32), y.view(torch.int32)), f"loss of call {i}: {float(x)} vs {float(y)}"
        assert torch.equal(a.flat_p.view(torch.int32), b.flat_p.view(torch.int32)), "the parameters differ"
        if accum == 1:   # the third batch of the epoch was the last
            with pytest.raises(IndexError):
                a.step_from(feed)
        wrong = ResidentDataset.from_frames(_samples["f"], 5, 3, DEV, shuffle=False)
        wrong.begin_epoch()
        with pytest.raises(RuntimeError, match="step_from: prepared for"):
            a.step_from(wrong)
    finally:
        for tr in (a, b):
            if tr is not None:
                tr.close()
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()


def test_validator_step_from_is_step_on_the_same_batches():
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    model = _model().eval()
    feed, twin = _feed(), _feed()
    feed.begin_epoch(), twin.begin_epoch()
    va = Validator(model, enRainfallLoss(0.57, 0.25, gamma=0.0), 20, 255.0)
    vb = Validator(model, enRainfallLoss(0.57, 0.25, gamma=0.0), 20, 255.0)
    try:
        # the first batch captures (into tensors of the feed's own), the later ones land in the graph's static buffers
        for n, more in ((2, 2), (3, 1)):
            for _ in range(more):
                out = va.step_from(feed)
                vb.step(*twin.fetch())
            torch.cuda.synchronize()
            assert float(va._block[1]) == n and float(va._block[0]) > 0
            assert torch.equal(va._block.view(torch.int64), vb._block.view(torch.int64)), f"the accumulator blocks differ after {n} batches"
        ent = next(iter(va._fwd._graphs.values()))
        assert out.data_ptr() == ent["out"].data_ptr()
        res = va.done(reset=True)
        assert (res["batches"], res["samples"], res["nonfinite"]) == (3, 6, 0)
        feed.begin_epoch(), twin.begin_epoch()   # after a reset the first batch takes the direct route at once
        va.step_from(feed)
        vb.done(reset=True)
        vb.step(*twin.fetch())
        torch.cuda.synchronize()
        assert torch.equal(va._block.view(torch.int64), vb._block.view(torch.int64))
    finally:
        va.close()
        vb.close()
