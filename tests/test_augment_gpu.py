"""The augmenting fetch on the GPU: adnm_batch_fetch_aug against the CPU yardstick (tests/augment_ref.py: torch's slicing,
flip and transpose), bit for bit, on its three paths (16-byte pieces, single floats, the transposing LDS tile), with crops at aligned and
misaligned offsets, with samples it must answer with NaNs, and with canaries round the destinations; then ResidentDataset(crop=,
augment=) over epochs, across a restore, and under FlatTrainer.step_from / Validator.step_from, bitwise."""
import pytest
import torch

import augment_ref
from adnm_hip import lib, ops, recipe
from adnm_hip.dataio import Augment, ResidentDataset, pack_word

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, T, T_IN, B = 5, 5, 2, 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


_stores = {}


def _store(Hs, Ws, n=N, t=T):
    """-> (the store on the host, the same on the device): random fp32 with a NaN payload, -0.0 and both infinities planted in every
    sample, made once per shape and never written"""
    key = (n, t, Hs, Ws)
    if key not in _stores:
        host = recipe.tensor(f"augment.store.{n}.{t}.{Hs}.{Ws}", (n, t, Hs, Ws)).clone()
        bits = host.view(torch.int32)
        for s in range(n):
            bits[s, 0, 0, 0] = 0x7FC12345                    # a quiet NaN with a payload
            bits[s, t - 1, Hs - 1, Ws - 1] = -2 ** 31        # -0.0
            host[s, 1, Hs // 2, Ws // 3] = float("inf")
            host[s, t - 2, Hs // 3, Ws // 2] = float("-inf")
        _stores[key] = (host, host.to(DEV))
    return _stores[key]


def _guarded(numel, lead):
    """-> (the whole allocation, NaN everywhere; the `numel` floats that start `lead` floats into it)"""
    whole = torch.full((lead + numel + 16,), float("nan"), device=DEV)
    return whole, whole[lead:lead + numel]


def _fetch_and_check(Hs, Ws, H, W, order, words, pos=0, batch=B, lead_x=16, lead_t=16, n=N, t=T, t_in=T_IN, expect_bad=None):
    """one launch into guarded destinations; every sample against the yardstick as bit patterns; nothing written outside"""
    host, dev = _store(Hs, Ws, n, t)
    order_t, words_t = torch.tensor(order, dtype=torch.int32), torch.tensor(words, dtype=torch.int64).to(torch.int32)
    wx, x = _guarded(batch * t_in * H * W, lead_x)
    wt, tgt = _guarded(batch * (t - t_in) * H * W, lead_t)
    order_d, words_d = order_t.to(DEV), words_t.to(DEV)
    lib.call("adnm_batch_fetch_aug", dev.data_ptr(), n, t, Hs, Ws, order_d.data_ptr(), words_d.data_ptr(), order_t.numel(), pos, x.data_ptr(), tgt.data_ptr(),
             batch, t_in, H, W, _stream())
    torch.cuda.synchronize()
    want_x, want_t, bad = augment_ref.batch(host, order_t, words_t, pos, batch, t_in, H, W)
    if expect_bad is not None:
        assert bad == list(expect_bad), "the yardstick itself"
    got_x, got_t = x.view(batch, t_in, H, W).cpu(), tgt.view(batch, t - t_in, H, W).cpu()
    for b in range(batch):
        what = f"sample {b} (index {order[pos + b]}, word {words[pos + b]:#x})"
        if b in bad:
            assert bool(torch.isnan(got_x[b]).all()) and bool(torch.isnan(got_t[b]).all()), what + " must be all NaN"
        else:
            assert augment_ref.same_bits(got_x[b], want_x[b]) and augment_ref.same_bits(got_t[b], want_t[b]), what + " differs from the yardstick"
    for whole, lead, numel in ((wx, lead_x, x.numel()), (wt, lead_t, tgt.numel())):
        assert bool(torch.isnan(whole[:lead]).all()) and bool(torch.isnan(whole[lead + numel:]).all()), "the fetch wrote outside its destination"
    return x, tgt


LEADS = [(16, 16), (17, 17)]   # 16-byte aligned destinations, and ones that are only 4-byte aligned (single floats on every sample)


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("S", [8, 9, 33])
def test_every_code_alone_and_mixed(S, lead):
    """8: 16-byte pieces; 9: single floats; 33: one full and three ragged transpose tiles.  One code per call, then identity, flip and
    transpose side by side in one batch, so that the per-sample branches are taken in one launch."""
    for code in range(8):
        _fetch_and_check(S, S, S, S, [3, 0, 4], [pack_word(code, 0, 0)] * 3, lead_x=lead[0], lead_t=lead[1])
    for codes in ((0, 1, 4), (6, 2, 3), (5, 7, 0)):
        _fetch_and_check(S, S, S, S, [9, 1, 1, 2, 0], [0] + [pack_word(c, 0, 0) for c in codes] + [0], pos=1, lead_x=lead[0], lead_t=lead[1])


@pytest.mark.parametrize("oy,ox", [(0, 0), (5, 4), (1, 1), (2, 3), (5, 5)])
def test_crops_of_a_45_store(oy, ox):
    """40 x 40 out of 45 x 45: Ws is odd, so every sample moves float by float; more than one transpose tile, ragged"""
    for code in range(8):
        _fetch_and_check(45, 45, 40, 40, [2, 4, 0], [pack_word(code, oy, ox), pack_word(code ^ 5, oy, ox), pack_word(code, ox, oy)])


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("oy,ox", [(0, 0), (4, 4), (1, 1), (2, 3), (4, 8)])
def test_crops_of_a_48_store(oy, ox, lead):
    """40 x 40 out of 48 x 48: W and Ws are multiples of 4, so the access width is the SAMPLE's: 16 bytes where ox % 4 == 0, floats
    where not, both in one launch"""
    for code in range(8):
        _fetch_and_check(48, 48, 40, 40, [2, 4, 0], [pack_word(code, oy, ox), pack_word(code ^ 3, 8, 8), pack_word(code, ox, oy)],
                         lead_x=lead[0], lead_t=lead[1])


@pytest.mark.parametrize("oy,ox", [(0, 0), (2, 4), (1, 3)])
def test_a_crop_that_is_not_square(oy, ox):
    for code in range(4):
        _fetch_and_check(10, 16, 8, 12, [1, 3, 3], [pack_word(code, oy, ox), pack_word(code ^ 1, 2, 4), pack_word(code ^ 2, 0, 0)])


@pytest.mark.parametrize("S", [8, 9])
def test_identity_words_equal_the_plain_fetch(S):
    host, dev = _store(S, S)
    order = torch.tensor([4, 1, 1, 0], dtype=torch.int32, device=DEV)
    x, tgt = _fetch_and_check(S, S, S, S, order.tolist(), [0, 0, 0, 0], pos=1)
    px, pt = torch.empty_like(x), torch.empty_like(tgt)
    lib.call("adnm_batch_fetch", dev.data_ptr(), N, T, S * S, order.data_ptr(), 4, 1, px.data_ptr(), pt.data_ptr(), B, T_IN, _stream())
    torch.cuda.synchronize()
    assert augment_ref.same_bits(x.cpu(), px.cpu()) and augment_ref.same_bits(tgt.cpu(), pt.cpu())


def test_the_steps_own_geometry():
    """128 x 128, B = 4, T = 25 out of a 136 x 136 store, random words: 100 workgroups per sample, every path in one launch"""
    words = Augment(seed=5).draw(8, 8, 8)
    assert len(set((words & 7).tolist())) >= 3
    _fetch_and_check(136, 136, 128, 128, [2, 0, 1, 2, 1, 0, 0, 2], words.tolist(), pos=2, batch=4, n=3, t=25, t_in=5)
    _fetch_and_check(128, 128, 128, 128, [2, 0, 1, 2], [pack_word(c, 0, 0) for c in (0, 3, 4, 7)], batch=4, n=3, t=25, t_in=5)


@pytest.mark.parametrize("S", [8, 9])
def test_a_sample_that_must_not_be_served_is_all_nan_and_its_neighbours_exact(S):
    Hs = S + 2
    ok = pack_word(1, 1, 1)
    for index, word in ((-1, ok), (N, ok), (2 ** 31 - 1, ok), (-2 ** 31, ok), (2, ok | (1 << 31)), (2, pack_word(0, 3, 0)), (2, pack_word(0, 0, 3)),
                        (2, pack_word(7, 16383, 16383)), (2, 0xFFFFFFFF)):
        _fetch_and_check(Hs, Hs, S, S, [1, index, 3], [pack_word(4, 2, 0), word, pack_word(2, 0, 2)], expect_bad=[1])
    torch.cuda.synchronize()   # no error from any launch


def test_the_transpose_bit_on_a_frame_that_is_not_square_gives_nans():
    _fetch_and_check(10, 16, 8, 12, [1, 2, 3], [pack_word(1, 0, 0), pack_word(4, 0, 0), pack_word(3, 2, 4)], expect_bad=[1])
    _fetch_and_check(10, 16, 8, 12, [1, 2, 3], [pack_word(7, 1, 1), pack_word(2, 1, 1), pack_word(5, 0, 0)], expect_bad=[0, 2])


# ------------------------------------------------------------------------------------------------ the feed
def _frames(n, t, Hs, Ws, name):
    return recipe.tensor(f"augment.frames.{name}", (n, t, Hs, Ws))


def _expected(frames, order, words, pos, batch, t_in, H, W):
    x, tgt, bad = augment_ref.batch(frames, order, words, pos, batch, t_in, H, W)
    assert not bad
    return x, tgt


def test_the_feed_serves_what_its_own_words_say_for_two_epochs():
    frames = _frames(7, 4, 20, 20, "feed")
    feed = ResidentDataset.from_frames(frames, 1, 2, DEV, generator=torch.Generator().manual_seed(21), crop=(16, 16), augment=Augment(seed=4))
    assert feed.x_shape == (2, 1, 1, 16, 16) and feed.tgt_shape == (2, 3, 1, 16, 16) and len(feed) == 3
    seen = []
    for epoch in range(2):
        feed.begin_epoch()
        order, words = feed.order.perm.clone(), feed.words.words.clone()
        seen.append(words)
        for step in range(len(feed)):
            x, tgt = feed.fetch()
            wx, wt = _expected(frames, order, words, step * 2, 2, 1, 16, 16)
            assert tuple(x.shape) == feed.x_shape and tuple(tgt.shape) == feed.tgt_shape
            assert augment_ref.same_bits(x[:, :, 0].cpu(), wx) and augment_ref.same_bits(tgt[:, :, 0].cpu(), wt), f"epoch {epoch} step {step}"
        with pytest.raises(IndexError):
            feed.fetch()
    assert not torch.equal(seen[0], seen[1])
    with pytest.raises(RuntimeError, match="fetch_into"):
        feed.begin_epoch()
        feed.fetch_into(torch.empty(2, 1, 1, 20, 20, device=DEV), torch.empty(2, 3, 1, 16, 16, device=DEV))
    with pytest.raises(ValueError, match="square"):
        ResidentDataset.from_frames(frames, 1, 2, DEV, crop=(16, 12), augment=Augment())


def test_ranks_serve_their_chunks_of_the_single_process_batch():
    frames = _frames(9, 3, 12, 12, "ranks")
    single = ResidentDataset.from_frames(frames, 1, 4, DEV, generator=torch.Generator().manual_seed(2), crop=(8, 8), augment=Augment(seed=9))
    ranks = [ResidentDataset.from_frames(frames, 1, 2, DEV, generator=torch.Generator().manual_seed(2), rank=r, world=2, crop=(8, 8),
                                         augment=Augment(seed=9)) for r in range(2)]
    for f in [single] + ranks:
        f.begin_epoch()
    for step in range(len(single)):
        x, tgt = single.fetch()
        parts = [f.fetch() for f in ranks]
        assert augment_ref.same_bits(x.cpu(), torch.cat([p[0] for p in parts]).cpu())
        assert augment_ref.same_bits(tgt.cpu(), torch.cat([p[1] for p in parts]).cpu())


def test_a_restored_augmenting_feed_goes_on_with_the_same_batches():
    frames = _frames(9, 3, 12, 12, "resume")

    def make(seed_order, seed_aug):
        return ResidentDataset.from_frames(frames, 1, 2, DEV, generator=torch.Generator().manual_seed(seed_order), crop=(8, 8),
                                           augment=Augment(seed=seed_aug))
    a = make(21, 7)
    a.begin_epoch()
    a.fetch()
    sd = a.state_dict()
    assert "augment" in sd
    b = make(5, 7)
    b.augment.draw(3, 1, 1)   # its generator stands elsewhere before the restore
    b.load_state_dict(sd)
    for _ in range(len(a) - 1):
        (xa, ta), (xb, tb) = a.fetch(), b.fetch()
        assert augment_ref.same_bits(xa.cpu(), xb.cpu()) and augment_ref.same_bits(ta.cpu(), tb.cpu())
    a.begin_epoch(), b.begin_epoch()
    assert torch.equal(a.words.words, b.words.words)
    assert augment_ref.same_bits(a.fetch()[0].cpu(), b.fetch()[0].cpu())
    plain = ResidentDataset.from_frames(frames, 1, 2, DEV, shuffle=False)
    plain.begin_epoch()
    with pytest.raises(ValueError, match='no "augment" key'):
        make(1, 1).load_state_dict(plain.state_dict())


def test_a_centre_crop_feed_equals_slicing():
    frames = _frames(5, 3, 13, 18, "centre")
    for augment in (None, Augment(flip_h=False, flip_v=False, transpose=False, shift=False)):
        feed = ResidentDataset.from_frames(frames, 2, 2, DEV, shuffle=False, crop=(8, 12), augment=augment)
        feed.begin_epoch()
        for step in range(len(feed)):
            x, tgt = feed.fetch()
            want = frames[2 * step:2 * step + 2, :, 2:10, 3:15]
            assert augment_ref.same_bits(x[:, :, 0].cpu(), want[:, :2]) and augment_ref.same_bits(tgt[:, :, 0].cpu(), want[:, 2:])
    assert "augment" not in ResidentDataset.from_frames(frames, 2, 2, DEV, crop=(8, 12)).state_dict()


def test_a_plain_feed_launches_the_plain_fetch_and_allocates_nothing(monkeypatch):
    frames = _frames(5, 3, 8, 8, "plain")
    names, call = [], lib.call

    def recorder(name, *args):
        names.append(name)
        return call(name, *args)
    with monkeypatch.context() as m:
        m.setattr(lib, "call", recorder)
        plain = ResidentDataset.from_frames(frames, 1, 2, DEV)
        plain.begin_epoch()
        plain.fetch(), plain.fetch()
        assert names == ["adnm_batch_fetch"] * 2
        assert plain.words is None and not hasattr(plain, "_words_dev") and set(plain.state_dict()) == set(plain.order.state_dict())
        del names[:]
        aug = ResidentDataset.from_frames(frames, 1, 2, DEV, augment=Augment())
        aug.begin_epoch()
        aug.fetch()
        assert names == ["adnm_batch_fetch_aug"]
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the consumers
def _model():
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(m)
    return m.to(DEV).train()


_samples = {}


def _feed(batch=2, augment=True):
    """a 72 x 72 store serving 64 x 64 (the size and batch of tests/test_feed_gpu.py::test_step_from_is_step_on_the_same_batches)"""
    if "f" not in _samples:
        _samples["f"] = recipe.radar_batch(6, 25, 72, name="augment.e2e")[:, :, 0].contiguous()
    return ResidentDataset.from_frames(_samples["f"], 5, batch, DEV, shuffle=True, generator=torch.Generator().manual_seed(3), crop=(64, 64),
                                       augment=Augment(seed=11) if augment else None)


def _trainer():
    from adnm_hip.trainer import FlatTrainer
    from models.loss import enRainfallLoss
    return FlatTrainer(_model(), enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025,
                       use_graph=True)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_step_from_an_augmenting_feed_is_step_on_the_same_batches(prec):
    ops.set_mfma_precision(prec)
    ops.QUANT.reset()
    a = b = None
    try:
        feed, twin = _feed(), _feed()
        feed.begin_epoch(), twin.begin_epoch()
        assert len(feed) == 3 and len(set((feed.words.words & 7).tolist())) > 1
        a, b = _trainer(), _trainer()
        la = [a.step_from(feed).detach().clone() for _ in range(3)]
        lb = [b.step(*twin.fetch()).detach().clone() for _ in range(3)]
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(la, lb)):
            assert bool(torch.isfinite(x)) and torch.equal(x.view(torch.int32), y.view(torch.int32)), f"loss of call {i}: {float(x)} vs {float(y)}"
        assert torch.equal(a.flat_p.view(torch.int32), b.flat_p.view(torch.int32)), "the parameters differ"
        # the twin's batches are the yardstick's: what the trainer stepped on is what the words say
        twin.begin_epoch()
        order, words = twin.order.perm.clone(), twin.words.words.clone()
        x, tgt = twin.fetch()
        wx, wt = _expected(_samples["f"], order, words, 0, 2, 5, 64, 64)
        assert augment_ref.same_bits(x[:, :, 0].cpu(), wx) and augment_ref.same_bits(tgt[:, :, 0].cpu(), wt)
    finally:
        for tr in (a, b):
            if tr is not None:
                tr.close()
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()


def test_validator_step_from_a_centre_crop_feed_is_step_on_the_sliced_tensors():
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    model = _model().eval()
    feed = _feed(augment=False)
    feed.begin_epoch()
    order = feed.order.perm.clone().long()
    va = Validator(model, enRainfallLoss(0.57, 0.25, gamma=0.0), 20, 255.0)
    vb = Validator(model, enRainfallLoss(0.57, 0.25, gamma=0.0), 20, 255.0)
    try:
        for step in range(3):   # the first batch captures, the later ones land in the graph's static buffers
            va.step_from(feed)
            sliced = _samples["f"][order[2 * step:2 * step + 2], :, 4:68, 4:68].unsqueeze(2).to(DEV)
            vb.step(sliced[:, :5].contiguous(), sliced[:, 5:].contiguous())
            torch.cuda.synchronize()
            assert float(va._block[1]) == step + 1
            assert torch.equal(va._block.view(torch.int64), vb._block.view(torch.int64)), f"the accumulator blocks differ after {step + 1} batches"
    finally:
        va.close()
        vb.close()
