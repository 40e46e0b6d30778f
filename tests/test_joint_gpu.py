"""The joint intensity histogram on the GPU (csrc/joint.hip: adnm_valid_joint_accum; ops.joint_histogram; Validator(joint=)): against
numpy.histogram2d on the quantised fields on the CPU (joint_ref), every comparison integer for integer; conservation; the hot bin; the
extreme levels; tails; addressing; accumulation and bit-reproducibility; the workspace contract; the counts the pooled pass gives; and
end to end through the captured graph."""
import numpy as np
import pytest
import torch

import joint_ref as J
from adnm_hip import lib, ops, recipe
from adnm_hip.validate import joint_counts_at, joint_entries

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (frames, T, H, W, scale): one pixel; a row shorter than a quad; an odd frame, a fractional scale; L = 2; L = 128, 64 KB of LDS;
# a frame of exactly one item of 4096 pixels
CASES = [(1, 1, 1, 1, 90.0), (2, 2, 1, 7, 90.0), (6, 2, 5, 13, 89.5), (4, 4, 16, 16, 1.0), (3, 1, 8, 33, 127.99), (6, 3, 64, 64, 90.0)]


def _case_id(c):
    return f"{c[0]}f-T{c[1]}-{c[2]}x{c[3]}-s{c[4]:g}"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _table(T, scale, tail=0):
    n = lib.query("adnm_valid_joint_block_bytes", T, scale) // 8
    assert n == T * J.levels(scale) ** 2
    return torch.zeros(n + tail, dtype=torch.float64, device=DEV)


def _accum(pred_ptr, sample_stride, frame_stride, tgt, table, T, scale, ws=None):
    """tgt: (frames, H, W) on the device, contiguous or a slice that is; the forecast by address and strides"""
    frames, hw = tgt.shape[0], tgt.shape[1] * tgt.shape[2]
    nb = lib.query("adnm_valid_joint_accum_ws_bytes", frames, T, hw, scale)
    assert nb >= 0
    if ws is None and nb:
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    lib.call("adnm_valid_joint_accum", pred_ptr, sample_stride, frame_stride, tgt.data_ptr(), table.data_ptr(), scale, None if ws is None else ws.data_ptr(), nb,
             frames, T, hw, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return nb


def _whole(table, T, L):
    """the (T, L, L) table as exact int64 on the host"""
    h = table[:T * L * L].cpu().numpy()
    assert (h == np.rint(h)).all() and (h >= 0).all(), "an entry is not a count"
    return h.astype(np.int64).reshape(T, L, L)


# ------------------------------------------------------------------------------------------------ 1. against the yardstick
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_joint_histogram_against_histogram2d(case):
    frames, T, H, W, scale = case
    L = J.levels(scale)
    t, p = J.sparse_fields(frames, H, W, 100 + frames + W)
    if H * W >= 64:
        assert np.isnan(t).any() and np.isinf(p).any() and (t < 0).any() and (p > 1).any(), "the planted values are not there"
        assert 0.8 < (t == 0).mean() < 0.95
    want = J.frame_hist(t, p, scale)
    got = ops.joint_histogram(_dev(t), _dev(p), scale)
    assert got.dtype == torch.int64 and tuple(got.shape) == (frames, L, L) and got.device.type == "cuda"
    assert (got.cpu().numpy() == want).all(), "one-shot, per frame"
    assert (got.sum(dim=(1, 2)).cpu().numpy() == H * W).all()
    table = _table(T, scale)
    pd = _dev(p)
    _accum(pd.data_ptr(), T * H * W, H * W, _dev(t), table, T, scale)
    rows = _whole(table, T, L)
    assert (rows == J.table(t, p, scale, T)).all(), "rows are frame indices f mod T"
    assert (rows.sum(axis=(1, 2)) == (frames // T) * H * W).all(), "conservation: every row sums to samples * H * W"
    four = ops.joint_histogram(_dev(t).view(frames // T, T, H, W), pd.view(frames // T, T, H, W), scale)
    assert torch.equal(four, got), "(B, T, H, W) is (frames, H, W)"


@pytest.mark.parametrize("scale", [90.0, 127.99])
def test_uniform_noise_over_all_levels(scale):
    frames, T, H, W = 4, 2, 96, 100
    L = J.levels(scale)
    t, p = J.uniform_fields(frames, H, W, 7)
    rows = _whole(_hist_table(t, p, T, scale), T, L)
    assert (rows == J.table(t, p, scale, T)).all()
    assert (rows.sum(axis=(1, 2)) == 2 * H * W).all() and (rows.sum(axis=0) > 0).mean() > 0.8, "most bins are hit"


def _hist_table(t, p, T, scale):
    table = _table(T, scale)
    pd, td = _dev(p), _dev(t)
    _accum(pd.data_ptr(), T * t.shape[1] * t.shape[2], t.shape[1] * t.shape[2], td, table, T, scale)
    return table


def test_more_items_than_workgroups():
    """T = 1 and 2100 frames: more items than the launch has workgroups, so some count two frames into one LDS histogram before they flush"""
    frames, H, W, scale = 2100, 4, 4, 90.0
    t, p = J.sparse_fields(frames, H, W, 5, plant=False)
    t[::3, 0, 0], p[::5, 1, 1] = 0.5, 0.25
    rows = _whole(_hist_table(t, p, 1, scale), 1, 91)
    assert (rows == J.table(t, p, scale, 1)).all() and rows.sum() == frames * H * W


# ------------------------------------------------------------------------------------------------ 2. the hot bin and the extreme levels
def test_an_all_zero_pair_lands_in_one_bin():
    """3 frames of 512 x 512, T = 1: 786 432 pixels in [0][0][0] — more than a 16-bit counter holds, all of them counted by ballot"""
    z = torch.zeros(3, 512, 512, dtype=torch.float32, device=DEV)
    table = _table(1, 90.0)
    _accum(z.data_ptr(), 512 * 512, 512 * 512, z, table, 1, 90.0)
    rows = _whole(table, 1, 91)
    assert rows[0, 0, 0] == 786432 and rows.sum() == 786432
    per_frame = ops.joint_histogram(z, z, 90.0)
    assert per_frame[:, 0, 0].tolist() == [262144] * 3 and int(per_frame.sum()) == 786432


@pytest.mark.parametrize("scale", [90.0, 1.0, 127.99, 89.5])
def test_extreme_levels_and_the_orientation(scale):
    L = J.levels(scale)
    zero, one = torch.zeros(2, 40, 50, dtype=torch.float32, device=DEV), torch.ones(2, 40, 50, dtype=torch.float32, device=DEV)
    both = ops.joint_histogram(one, one, scale)
    assert both[:, L - 1, L - 1].tolist() == [2000, 2000] and int(both.sum()) == 4000
    miss = ops.joint_histogram(zero, one, scale)          # target zero, forecast one: row 0, column L - 1
    assert miss[:, 0, L - 1].tolist() == [2000, 2000] and int(miss.sum()) == 4000 and int(miss[:, L - 1, 0].sum()) == 0
    inf = ops.joint_histogram(one * float("inf"), one * float("-inf"), scale)
    assert inf[:, L - 1, 0].tolist() == [2000, 2000]
    nan = ops.joint_histogram(one * float("nan"), one * 5.0, scale)
    assert nan[:, 0, L - 1].tolist() == [2000, 2000]


# ------------------------------------------------------------------------------------------------ 3. tails
@pytest.mark.parametrize("hw", [63, 64, 65, 257, 1000, 4095, 4097, 8196])
def test_tails_with_the_last_pixel_non_zero(hw):
    """the last pixels of a wave, of a quad and of an item; 4097 and 8196 give an item of one pixel and one of one quad"""
    frames, T, scale = 4, 2, 90.0
    t, p = np.zeros((frames, 1, hw), dtype=np.float32), np.zeros((frames, 1, hw), dtype=np.float32)
    t[:, 0, -1], p[:, 0, -1] = 0.5, 0.25
    t[1, 0, hw // 2], p[2, 0, 0] = 1.0, 0.75
    rows = _whole(_hist_table(t, p, T, scale), T, 91)
    assert (rows == J.table(t, p, scale, T)).all()
    assert rows[:, 45, 22].tolist() == [2, 2] and rows.sum() == frames * hw


# ------------------------------------------------------------------------------------------------ 4. addressing
@pytest.mark.parametrize("H,W", [(8, 12), (64, 68)])
def test_a_base_one_float_off_takes_the_scalar_route_with_the_same_table(H, W):
    B, T, scale = 2, 2, 90.0
    tn, pn = J.sparse_fields(B * T, H, W, 31)
    tgt, pred = _dev(tn), _dev(pn)
    want = _table(T, scale)
    _accum(pred.data_ptr(), T * H * W, H * W, tgt, want, T, scale)
    assert (_whole(want, T, 91) == J.table(tn, pn, scale, T)).all()
    hold_p, hold_t = (torch.zeros(B * T * H * W + 1, dtype=torch.float32, device=DEV) for _ in range(2))
    off_p, off_t = hold_p[1:].view(B * T, H, W), hold_t[1:].view(B * T, H, W)
    off_p.copy_(pred), off_t.copy_(tgt)
    assert off_p.data_ptr() % 16 == 4 and off_t.data_ptr() % 16 == 4 and pred.data_ptr() % 16 == 0 and tgt.data_ptr() % 16 == 0
    got = _table(T, scale)
    _accum(off_p.data_ptr(), T * H * W, H * W, off_t, got, T, scale)
    assert torch.equal(_bits(got), _bits(want)), "float-by-float loads give another table than 16-byte loads"
    wide = torch.full((B, T + 2, H, W), 0.9, dtype=torch.float32, device=DEV)
    wide[:, 1:T + 1] = pred.view(B, T, H, W)
    got = _table(T, scale)
    _accum(wide[:, 1:].data_ptr(), (T + 2) * H * W, H * W, tgt, got, T, scale)
    assert torch.equal(_bits(got), _bits(want)), "a slice of a wider tensor"


def test_a_held_frame_is_the_materialised_repeat():
    B, T, T_in, H, W, scale = 2, 3, 2, 16, 20, 90.0
    tn = J.sparse_fields(B * T, H, W, 21)[0]
    xn = J.sparse_fields(B * T_in, H, W, 22)[1]
    t, x = _dev(tn), _dev(xn).view(B, T_in, H, W)
    a, b = _table(T, scale), _table(T, scale)
    _accum(x.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, t, a, T, scale)          # the last input frame, held over the horizon
    held = x[:, -1:].expand(B, T, H, W).contiguous().view(B * T, H, W)
    _accum(held.data_ptr(), T * H * W, H * W, t, b, T, scale)
    assert torch.equal(_bits(a), _bits(b))
    assert (_whole(a, T, 91) == J.table(tn, held.cpu().numpy(), scale, T)).all()


# ------------------------------------------------------------------------------------------------ 5. accumulation
def test_two_calls_add_and_two_runs_give_equal_bits():
    B, T, H, W, scale = 2, 2, 32, 36, 90.0
    batches = [J.sparse_fields(B * T, H, W, seed) for seed in (11, 12)]
    one = [J.table(t, p, scale, T) for t, p in batches]
    assert (one[0] != J.frame_hist(*batches[0], scale).reshape(T, B, 91, 91).sum(1)).any(), "f mod T and f / T coincide on this data: nothing is tested"
    tables = []
    for _ in range(2):
        table = _table(T, scale)
        for i, (t, p) in enumerate(batches):
            pd = _dev(p)
            _accum(pd.data_ptr(), T * H * W, H * W, _dev(t), table, T, scale)
            assert (_whole(table, T, 91) == sum(one[:i + 1])).all(), f"after batch {i}"
        tables.append(table)
    assert torch.equal(_bits(tables[0]), _bits(tables[1])), "the same calls on a fresh table give other bits"
    again = [ops.joint_histogram(_dev(batches[0][0]), _dev(batches[0][1]), scale) for _ in range(2)]
    assert torch.equal(again[0], again[1])


# ------------------------------------------------------------------------------------------------ 6. the workspace contract
def test_the_workspace_and_what_lies_behind_it_and_behind_the_table():
    """with a query of 0 the call takes a null workspace, and a buffer handed to it all the same stays untouched; with a non-zero query the
    result does not depend on what the workspace held and nothing behind ws_bytes is written"""
    B, T, H, W, scale = 2, 3, 24, 20, 90.0
    tn, pn = J.sparse_fields(B * T, H, W, 41)
    tgt, pred = _dev(tn), _dev(pn)
    nb = lib.query("adnm_valid_joint_accum_ws_bytes", B * T, T, H * W, scale)
    cells, guard = T * 91 * 91, 4096
    results = []
    for fill in (0x00, 0xFF):
        ws = torch.full((nb + guard,), fill, dtype=torch.uint8, device=DEV)
        ws[nb:] = 0xA5
        hold = torch.full((cells + 64,), -7.0, dtype=torch.float64, device=DEV)
        hold[:cells] = 0.0
        assert _accum(pred.data_ptr(), T * H * W, H * W, tgt, hold, T, scale, ws=ws) == nb
        assert bool((ws[nb:] == 0xA5).all()), "a write behind ws_bytes"
        assert bool((hold[cells:] == -7.0).all()), "a write behind the table"
        results.append(hold[:cells].clone())
    assert torch.equal(_bits(results[0]), _bits(results[1])), "the result depends on what the workspace held"
    assert (_whole(results[0], T, 91) == J.table(tn, pn, scale, T)).all()
    if nb == 0:
        bare = _table(T, scale)
        _accum(pred.data_ptr(), T * H * W, H * W, tgt, bare, T, scale, ws=None)          # a null workspace
        assert torch.equal(_bits(bare), _bits(results[0]))


# ------------------------------------------------------------------------------------------------ 7. the counts the project already has
def test_the_histogram_gives_the_pooled_pass_its_counts():
    frames, H, W, scale = 4, 48, 52, 90.0
    thr = (20, 30, 35, 40, 27.5)
    t = (np.clip(J.sparse_fields(frames, H, W, 51)[0], 0, None) * 0.6).astype(np.float32)
    p = (np.clip(J.sparse_fields(frames, H, W, 52, plant=False)[0], 0, None) * 0.5 + t * 0.5).astype(np.float32)
    td, pd = _dev(t), _dev(p)
    hist = ops.joint_histogram(td, pd, scale)
    counts = ops.pool_counts(td, pd, thr, scale, pools=((1, 1),)).cpu().numpy()[:, 0]          # (frames, 4 * nthr): TP, FN, FP, TN per threshold
    for k, v in enumerate(thr):
        got = np.stack(joint_counts_at(hist, v), axis=1)
        assert (got == counts[:, 4 * k:4 * k + 4]).all(), v
        assert got[:, :3].sum() > 0, f"no event at {v}: nothing is compared"
    assert (np.stack(joint_counts_at(hist, 27.5), 1) == np.stack(joint_counts_at(hist, 28), 1)).all()


# ------------------------------------------------------------------------------------------------ 8. the Validator end to end
def _model():
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(m)
    return m.to(DEV).eval()


def _same_tree(a, b):
    """bitwise: dictionaries key for key in order, arrays and numbers value for value with NaN equal to NaN"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same_tree(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(((a == b) | ((a != a) & (b != b))).all())


def test_validator_with_joint_end_to_end():
    import spectrum_ref as S
    from adnm_hip.validate import Validator, joint_doubles
    from models.loss import enRainfallLoss
    model, crit, scale, T, thr, L = _model(), enRainfallLoss(0.57, 0.25, gamma=0.0), 90.0, 20, [20, 30, 35, 40], 91
    rng = np.random.default_rng(3)
    frames = np.stack([S.fields(25, 64, 64, 3, 50 + i)[0] for i in range(4)]).clip(0, 1) * 0.45 + rng.normal(0, 0.004, (4, 25, 64, 64))
    samples = _dev(frames.astype(np.float32))
    data = [(samples[i:i + 2, :5, None].contiguous(), samples[i:i + 2, 5:, None].contiguous()) for i in (0, 2)]
    kw = dict(spectrum=True, pools=(4,), fss=(5,), persistence=True, advection=True)
    val = Validator(model, crit, T, scale, thr, joint=True, **kw)
    former = Validator(model, crit, T, scale, thr, **kw)
    try:
        assert joint_doubles(T, scale) == T * L * L
        hist = torch.zeros(T, L, L, dtype=torch.int64, device=DEV)
        for x, tgt in data:            # two steps through the captured graph
            val.step(x, tgt)
            ent = val._fwd.entry(x)
            hist += ops.joint_histogram(ent["tgt"], ent["pred"].view(2, T, 64, 64), scale).view(2, T, L, L).sum(0)
            former.step(x, tgt)
        hist = hist.cpu().numpy()
        # with joint=False nothing is there: the old length, no workspace, no key
        assert val._block.numel() == former._block.numel() + T * L * L and former.joint is False
        assert (_whole(val._block[-T * L * L:], T, L) == hist).all(), "the table at the end of the one allocation"
        assert torch.equal(_bits(val._block[:-T * L * L]), _bits(former._block)), "a former offset moved, or a former pass counts differently"
        res, old = val.done(per_lead=True), former.done(per_lead=True)
        assert "joint" not in old and "joint" not in old["per_lead"]
        assert list(res) == list(old)[:-1] + ["joint", "per_lead"] and list(res["per_lead"]) == list(old["per_lead"]) + ["joint"]
        assert _same_tree({k: res[k] for k in old if k != "per_lead"}, {k: old[k] for k in old if k != "per_lead"}), "a former entry moved"
        assert _same_tree({k: res["per_lead"][k] for k in old["per_lead"]}, old["per_lead"]), "a former per-lead entry moved"
        j, lead = res["joint"], res["per_lead"]["joint"]
        assert j["levels"] == L and (j["histogram"] == hist.sum(0)).all() and (lead["histogram"] == hist).all()
        assert _same_tree(j, joint_entries(hist.sum(0))) and _same_tree(lead, joint_entries(hist))
        assert int(j["histogram"].sum()) == 4 * T * 64 * 64 and (lead["histogram"].sum(axis=(1, 2)) == 4 * 64 * 64).all()
        assert (res["samples"], res["batches"]) == (4, 2)
        for v in thr:
            for k in ("TP", "FN", "FP", "TN"):
                assert res["threshold_metrics"][v][k] == j["curves"][k][v], (v, k)
                assert (res["per_lead"]["threshold_metrics"][v][k] == lead["curves"][k][:, v]).all(), (v, k)
        assert j["curves"]["TP"][20] + j["curves"]["FN"][20] > 0, "no observed event at 20: the comparison is empty"
        print("joint end to end: bias at 5, 20, 30:", j["curves"]["bias"][[5, 20, 30]], "correlation", j["correlation"], "mean error", j["mean_error"])
        # once the graph exists a step allocates nothing
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        val.step(*data[0])
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        val.reset()
        assert float(val._block[-T * L * L:].abs().sum()) == 0.0 and float(val._block.abs().sum()) == 0.0, "reset() zeroes the tail"
        val.step(*data[0])
        first = ops.joint_histogram(val._fwd.entry(data[0][0])["tgt"], val._fwd.entry(data[0][0])["pred"].view(2, T, 64, 64), scale).view(2, T, L, L).sum(0)
        assert (val.done()["joint"]["histogram"] == first.sum(0).cpu().numpy()).all(), "after reset() the epoch starts from zero"
    finally:
        val.close()
        former.close()


def test_a_value_scale_outside_the_limits_raises_in_the_constructor():
    from adnm_hip.validate import Validator
    from models.loss import RainfallLoss
    with pytest.raises(ValueError, match="2 <= floor"):
        Validator(torch.nn.Identity(), RainfallLoss(), 20, 255.0, joint=True)
    with pytest.raises(ValueError, match="2 <= floor"):
        ops.joint_histogram(torch.zeros(1, 8, 8, device=DEV), torch.zeros(1, 8, 8, device=DEV), 255.0)
