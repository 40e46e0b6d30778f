"""The host side of the augmenting feed, without a GPU: the word layout, the eight symmetries under the yardstick, what
Augment draws and from where (the order must stay the DataLoader's), the split over ranks, the state, and adnm_batch_fetch_aug at the C
boundary (declared, exported, additive, refusing bad arguments before any launch)."""
import ctypes
import io

import pytest
import torch
from torch.utils.data import DataLoader

import augment_ref
from adnm_hip import lib
from adnm_hip.dataio import Augment, EpochOrder, EpochWords, ResidentDataset, pack_word, unpack_word


# ------------------------------------------------------------------------------------------------ the word
@pytest.mark.parametrize("code,oy,ox", [(0, 0, 0), (7, 16383, 0), (5, 0, 16383), (7, 16383, 16383), (2, 5, 4)])
def test_word_round_trip_at_the_field_limits(code, oy, ox):
    w = pack_word(code, oy, ox)
    assert 0 <= w < 2 ** 31, "bit 31 stays clear"
    assert unpack_word(w) == (code, oy, ox)
    assert augment_ref.decode(w) == (bool(code & 1), bool(code & 2), bool(code & 4), oy, ox, False), "the header's table, read independently"
    t = pack_word(torch.tensor([code]), torch.tensor([oy]), torch.tensor([ox]))
    assert t.dtype == torch.int32 and int(t[0]) == w
    assert [int(v[0]) for v in unpack_word(t)] == [code, oy, ox]


def test_word_fields_outside_their_limits_are_refused():
    for bad in ((8, 0, 0), (0, 16384, 0), (0, 0, 16384), (-1, 0, 0), (0, -1, 0)):
        with pytest.raises(ValueError):
            pack_word(*bad)
    with pytest.raises(ValueError):
        pack_word(torch.tensor([0, 1]), torch.tensor([0, 16384]), torch.tensor([0, 0]))


def test_the_eight_codes_give_eight_different_images():
    frame = torch.arange(16, dtype=torch.float32).view(1, 4, 4)
    images = [augment_ref.served(frame, pack_word(c, 0, 0), 4, 4) for c in range(8)]
    assert len({tuple(i.flatten().tolist()) for i in images}) == 8
    assert torch.equal(images[0], frame)
    assert torch.equal(images[1][0, 0], torch.tensor([3., 2., 1., 0.])), "bit 0 reverses the rows' elements"
    assert torch.equal(images[2][0, 0], torch.tensor([12., 13., 14., 15.])), "bit 1 reverses the rows' order"
    assert torch.equal(images[4][0, 0], torch.tensor([0., 4., 8., 12.])), "bit 2 turns columns into rows"
    assert torch.equal(images[7][0, 0], torch.tensor([15., 11., 7., 3.])), "both flips come before the transpose"


# ------------------------------------------------------------------------------------------------ the draws
def test_draw_covers_codes_and_offsets_and_is_reproducible():
    w = Augment(seed=0).draw(64, 5, 5)
    assert w.dtype == torch.int32 and tuple(w.shape) == (64,)
    code, oy, ox = unpack_word(w)
    assert torch.bincount(code, minlength=8).tolist() == [10, 9, 5, 12, 5, 6, 6, 11], "torch's randint stream for seed 0"
    assert sorted(set(oy.tolist())) == sorted(set(ox.tolist())) == [0, 1, 2, 3, 4, 5]
    assert torch.equal(w, Augment(seed=0).draw(64, 5, 5)), "the same seed gives the same words"
    assert not torch.equal(w, Augment(seed=1).draw(64, 5, 5))
    # the documented sequence of draws, on a generator of the test's own
    g = torch.Generator().manual_seed(0)
    want = pack_word(torch.randint(0, 8, (64,), generator=g), torch.randint(0, 6, (64,), generator=g), torch.randint(0, 6, (64,), generator=g))
    assert torch.equal(w, want)


def test_two_consecutive_epochs_differ():
    words = EpochWords(64, 5, 5, Augment(seed=3))
    first = words.next_epoch().clone()
    assert not torch.equal(first, words.next_epoch())


def test_masks_and_the_centre_offset():
    code = unpack_word(Augment(flip_v=False, seed=2).draw(256, 3, 3))[0]
    assert not bool((code & 2).any()) and bool((code & 1).any()) and bool((code & 4).any())
    code = unpack_word(Augment(flip_h=False, transpose=False, seed=2).draw(256, 3, 3))[0]
    assert set(code.tolist()) == {0, 2}
    a = Augment(shift=False, seed=2)
    code, oy, ox = unpack_word(a.draw(256, 32, 7))
    assert set(oy.tolist()) == {16} and set(ox.tolist()) == {3} and len(set(code.tolist())) == 8
    # nothing was drawn for the offsets: the next codes are the generator's next draw
    g = torch.Generator().manual_seed(2)
    torch.randint(0, 8, (256,), generator=g)
    assert torch.equal(unpack_word(a.draw(16, 32, 7))[0], torch.randint(0, 8, (16,), generator=g))
    # no Augment at all: the centre window, untransformed, every epoch
    plain = EpochWords(5, 32, 7)
    assert plain.next_epoch().tolist() == [pack_word(0, 16, 3)] * 5 and plain.next_epoch().dtype == torch.int32


# ------------------------------------------------------------------------------------------------ the order stays the loader's
def _loader_epochs(n, batch, epochs, generator=None):
    data = [torch.tensor([i]) for i in range(n)]
    loader = DataLoader(data, batch_size=batch, shuffle=True, drop_last=True, generator=generator)
    return [[b.flatten().tolist() for b in loader] for _ in range(epochs)]


def _feed_epochs(order, words, epochs):
    """what ResidentDataset.begin_epoch does on the host: the order first, then the words"""
    out = []
    for _ in range(epochs):
        order.next_epoch()
        words.next_epoch()
        out.append([order.next_batch().tolist() for _ in range(len(order))])
    return out


def test_order_beside_an_augment_equals_the_real_loader_with_an_explicit_generator():
    g1, g2 = torch.Generator().manual_seed(1234), torch.Generator().manual_seed(1234)
    want = _loader_epochs(11, 4, 3, generator=g1)
    got = _feed_epochs(EpochOrder(11, 4, generator=g2), EpochWords(11, 5, 5, Augment(seed=1234)), 3)
    assert got == want and want[0] != want[1]
    assert torch.equal(g1.get_state(), g2.get_state())


def test_order_beside_an_augment_equals_the_real_loader_with_the_default_generator():
    torch.manual_seed(77)
    want = _loader_epochs(11, 4, 3)
    state = torch.get_rng_state()
    torch.manual_seed(77)
    got = _feed_epochs(EpochOrder(11, 4), EpochWords(11, 5, 5, Augment(seed=77)), 3)
    assert got == want
    assert torch.equal(state, torch.get_rng_state()), "the default generator ends where the loader leaves it: Augment never drew from it"


def test_ranks_read_their_chunk_of_the_single_process_words():
    n, B, world = 26, 2, 2
    single_o, single_w = EpochOrder(n, B * world, generator=torch.Generator().manual_seed(5)), EpochWords(n, 4, 4, Augment(seed=8))
    ranks = [(EpochOrder(n, B, generator=torch.Generator().manual_seed(5), rank=r, world=world), EpochWords(n, 4, 4, Augment(seed=8)))
             for r in range(world)]
    for epoch in range(2):
        single_o.next_epoch(), single_w.next_epoch()
        for o, w in ranks:
            o.next_epoch(), w.next_epoch()
        for g in range(len(single_o)):
            lo = single_o.offset(g)
            whole_idx, whole_w = single_o.perm[lo:lo + B * world], single_w.words[lo:lo + B * world]
            for r, (o, w) in enumerate(ranks):
                at = o.offset(g)
                assert torch.equal(o.perm[at:at + B], whole_idx[r * B:(r + 1) * B])
                assert torch.equal(w.words[at:at + B], whole_w[r * B:(r + 1) * B]), f"epoch {epoch} step {g} rank {r}"


# ------------------------------------------------------------------------------------------------ the state
def test_state_round_trip_and_a_state_without_the_key():
    order, words = EpochOrder(11, 2, generator=torch.Generator().manual_seed(9)), EpochWords(11, 3, 2, Augment(flip_v=False, seed=6))
    order.next_epoch(), words.next_epoch()
    order.next_epoch(), words.next_epoch()
    order.next_batch()
    sd = words.state_into(order.state_dict())
    assert set(sd["augment"]) == {"spec", "words", "generator"} and sd["augment"]["spec"]["seed"] == 6
    buf = io.BytesIO()
    torch.save({"feed": sd}, buf)
    buf.seek(0)
    sd = torch.load(buf)["feed"]
    twin = EpochWords(11, 3, 2, Augment(flip_v=False, seed=6))
    twin.augment.draw(5, 1, 1)   # anywhere else in its stream
    twin.load_from(sd)
    assert torch.equal(twin.words, words.words)
    assert torch.equal(twin.next_epoch(), words.next_epoch()), "the generator goes on where the saved one stood"
    plain = order.state_dict()
    assert "augment" not in plain and set(EpochWords(11, 3, 2).state_into(dict(plain))) == set(plain), "without an Augment the state is the order's"
    with pytest.raises(ValueError, match='no "augment" key'):
        twin.load_from(plain)
    with pytest.raises(ValueError, match="saved with augmentation"):
        EpochWords(11, 3, 2, Augment(seed=6)).load_from(sd)
    with pytest.raises(ValueError, match="has no Augment"):
        EpochWords(11, 3, 2).load_from(sd)


def test_the_constructor_refuses_what_the_kernel_would_not_serve():
    assert ResidentDataset._served(160, 160, (128, 128), Augment()) == (128, 128)
    assert ResidentDataset._served(10, 16, (8, 12), Augment(transpose=False)) == (8, 12)
    assert ResidentDataset._served(10, 16, None, None) == (10, 16)
    with pytest.raises(ValueError, match="square"):
        ResidentDataset._served(10, 16, (8, 12), Augment())
    with pytest.raises(ValueError, match="crop"):
        ResidentDataset._served(10, 16, (11, 12), None)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_batch_fetch_aug_is_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    assert "adnm_batch_fetch_aug" in protos, "adnm_batch_fetch_aug is not declared in include/adnm_hip.h"
    assert hasattr(so, "adnm_batch_fetch_aug"), "adnm_batch_fetch_aug declared but not exported"
    ret, args = protos["adnm_batch_fetch_aug"]
    assert ret == "int" and args[-1] == "adnm_stream_t" and args[5] == args[6] == "const int32_t*" and len(args) == 16
    assert len(protos["adnm_batch_fetch"][1]) == 12, "adnm_batch_fetch keeps its prototype"
    assert lib.load().adnm_abi_version() == 11


def test_batch_fetch_aug_checks_its_arguments_on_the_host():
    f = lib.load().adnm_batch_fetch_aug
    p = 4096   # stands for a device address: nothing is dereferenced or launched before a refusal

    def refused(what, store=p, n=7, T=5, Hs=10, Ws=12, order=p, aug=p, olen=7, pos=0, x=p, tgt=p, B=3, T_in=2, H=8, W=8):
        assert f(store, n, T, Hs, Ws, order, aug, olen, pos, x, tgt, B, T_in, H, W, None) == -1, what
        return lib.last_error()

    for k in ("store", "order", "aug", "x", "tgt"):
        assert "null pointer" in refused(k, **{k: None})
        assert "4-byte aligned" in refused(k + " at an odd address", **{k: p + 2})
    assert "batch must be in [1, 65535]" in refused("B = 0", B=0)
    assert "batch must be in [1, 65535]" in refused("B over the grid limit", B=65536, olen=1 << 20, n=1 << 20)
    assert "T_in must be in [1, T)" in refused("T_in = 0", T_in=0)
    assert "T_in must be in [1, T)" in refused("T_in = T", T_in=5)
    assert "T_in must be in [1, T)" in refused("T_in > T", T_in=6)
    for k in ("H", "W", "Hs", "Ws"):
        assert "[1, 16384)" in refused(k + " = 0", **{k: 0})
        assert "[1, 16384)" in refused(k + " = 16384", **{k: 16384, "Hs": 16384, "Ws": 16384} if k in ("H", "W") else {k: 16384})
    assert "larger than the stored" in refused("H > Hs", H=11)
    assert "larger than the stored" in refused("W > Ws", W=13)
    assert "2^31" in refused("a sample of more than 2^31 floats", T=9, Hs=16383, Ws=16383)   # 9 * 16383^2 = 2.4e9
    assert "outside an order" in refused("pos < 0", pos=-1)
    assert "outside an order" in refused("pos near the end of int64", pos=(1 << 63) - 2)
    assert "outside an order" in refused("pos + B > order_len", pos=5)
    assert "outside an order" in refused("order_len < B", olen=2)
    assert "[1, 2^31)" in refused("n_samples = 2^31", n=1 << 31)
    assert "[1, 2^31)" in refused("order_len = 2^31", olen=1 << 31)
    assert "[1, 2^31)" in refused("order_len = 0", olen=0)
