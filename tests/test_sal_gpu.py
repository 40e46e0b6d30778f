"""Per-object intensity moments and the SAL scores on the GPU (csrc/sal.hip: adnm_object_moments, adnm_valid_sal_accum; ops.object_moments,
ops.sal_table; Validator(sal=)) against scipy.ndimage on the CPU (sal_ref).  The moments are compared integer for integer, every element of
the output; the count columns of the SAL rows exactly and every per-frame A, S, L1, L2 and L within 1e-10 absolute.  That bar is derived, not
measured: the integer stage is exact, V >= 1, each sum has at most 16 384 non-negative terms, so its relative error is at most
16 384 * 2^-53 = 1.8e-12 in any order, and S and L2 amplify that by at most 4.

Frames of 114 x 116 are the largest whose records and words both live in LDS, 115 x 115 the first whose records use the workspace,
161 x 161 the last whose words live in LDS, 162 x 162 the first that keep both in the workspace, 256 x 256 the limit."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import sal_ref as S
from adnm_hip import lib, ops
from util import guarded_workspaces, poisoned_outputs, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE, TOL = 90.0, 1e-10
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (16, 16), (33, 65), (64, 64), (114, 116), (115, 115), (130, 129), (161, 161), (162, 162), (200, 200),
         (256, 256)]
TIERS = [(64, 64), (130, 129), (200, 200)]          # one frame per place the records and the words can live
SWITCHES = [(114, 116), (115, 115), (161, 161), (162, 162)]          # the frames on each side of the two switches: the item kernel at a full LDS
ONES = [0] + [1] * 90                               # every level above 0 weighs 1: R is an area
TOP = list(range(90)) + [65535]                     # the largest weight at the top level
WEIGHTS = {"identity": None, "ones": ONES, "top": TOP}
SCORES = [1, 2, 4, 6, 7, 8, 9]
COUNTS = [0, 3, 5, 10, 11]
seen = {}          # what -> the largest deviation of that comparison, for the record (_deviation_record)


@pytest.fixture(scope="module", autouse=True)
def _deviation_record():
    """profiles/sal_error.txt: with ADNM_SAL_ERROR_OUT=<path> in the environment the deviations this module's comparisons saw are written
    there when its last test has run (ADNM_SAL_ERROR_OUT=profiles/sal_error.txt python -m pytest -m gpu tests/test_sal_gpu.py); without
    it nothing is written.  Every comparison asserts the bar itself (_compare_rows): the record adds no check."""
    yield
    out = os.environ.get("ADNM_SAL_ERROR_OUT")
    if out and seen:
        head = ("tests/test_sal_gpu.py, one run: the largest absolute difference between a device score (A, |A|, L1, S, |S|, L2, L of one frame pair and\n"
                "threshold, or of a folded table) and the float64 yardstick's (tests/sal_ref.py), case by case.  The bar is 1e-10, derived and not measured:\n"
                "the integer stage is exact, V >= 1, a sum has at most 16 384 non-negative terms (relative error at most 16 384 * 2^-53 = 1.8e-12 in any\n"
                "order), and S and L2 amplify that by at most 4.\n")
        with open(out, "w") as f:
            f.write(head + "".join(f"  {what}: {dev:.3e}\n" for what, dev in seen.items()) + f"  largest: {max(seen.values()):.3e} (bar {TOL:.0e})\n")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _shift(a, dy, dx):
    """the field moved by (dy, dx) >= 0, zeros coming in"""
    out = np.zeros_like(a)
    H, W = a.shape[-2:]
    out[..., dy:, dx:] = a[..., :H - dy, :W - dx]
    return out


def _ragged(pattern, seed):
    """a 0 / 1 pattern with every event at its own level in 45 .. 89 (the events at a threshold of 20 stay the pattern)"""
    amp = np.random.default_rng(seed).uniform(0.51, 0.99, pattern.shape)
    return (pattern * amp).astype(np.float32)


def _check_moments(field, thr=20.0, scale=SCALE, min_area=1, intensity=None):
    """(frames, H, W) numpy field: every element of the moments image, integer for integer -> the image"""
    field = np.asarray(field, dtype=np.float32)
    fd = _dev(field)
    got = ops.object_moments(fd, thr, scale, min_area, intensity)
    assert got.dtype == torch.int64 and tuple(got.shape) == (field.shape[0], 4) + field.shape[1:] and got.device.type == "cuda"
    host = got.cpu().numpy()
    want = S.moments(field, thr, scale, min_area, intensity)
    bad = np.argwhere(host != want)
    assert bad.size == 0, f"(frame, moment, y, x) {bad[:8].tolist()}: got {host[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    lab = ops.label_objects(fd, thr, scale, min_area).cpu().numpy()
    first = lab == np.arange(1, lab[0].size + 1).reshape(lab.shape[1:])
    assert not (host * ~first[:, None]).any(), "a moment away from an object's first pixel"
    return host


# ------------------------------------------------------------------------------------------------ 1. object_moments: sizes and patterns
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_moments_of_the_patterns_at_every_size(H, W):
    """one frame per pattern, every event at its own level: empty, full, checkerboard, lattice, comb, serpentine, a spiral where the frame is
    square, and a full frame at the top level"""
    pats = [np.zeros((H, W), np.float32), np.ones((H, W), np.float32), S.checkerboard(H, W), S.lattice(H, W), S.comb(H, W), S.serpentine(H, W)]
    if H == W:
        pats.append(S.spiral(H))
    field = np.stack([_ragged(p, 7 + i) for i, p in enumerate(pats)] + [np.ones((H, W), np.float32)])
    got = _check_moments(field)
    assert not got[0].any(), "an empty frame has no moments"
    assert (got[1:, 0] > 0).sum(axis=(1, 2)).tolist()[:2] == [1, 1 if min(H, W) > 1 else (max(H, W) + 1) // 2], "full and checkerboard"
    assert (got[3, 0] > 0).sum() == ((H + 1) // 2) * ((W + 1) // 2), "the lattice uses every record"
    assert got[-1, :, 0, 0].tolist() == [90 * H * W, 90, 90 * H * (W - 1) * W // 2, 90 * W * (H - 1) * H // 2] and not got[-1, :, 1:, 1:].any()
    if (H, W) == (256, 256):
        top = _check_moments(field[-1:], intensity=TOP)[0]
        assert top[:, 0, 0].tolist() == [65535 * 65536, 65535, 65535 * 256 * 255 * 128, 65535 * 256 * 255 * 128], "the largest R, X and Y a frame can give"


@pytest.mark.parametrize("n", [32, 128])
def test_a_spiral_is_one_object(n):
    got = _check_moments(_ragged(S.spiral(n), 3)[None])
    assert (got[0, 0] > 0).sum() == 1 and got[0, 0, 0, 0] > 0


def test_a_frame_above_the_limit_raises():
    z = torch.zeros(1, 257, 256, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="65536"):
        ops.object_moments(z, 20.0, SCALE)
    with pytest.raises(RuntimeError, match="65536"):
        ops.sal_table(z, z, (20.0,), SCALE)
    small = z[:, :8, :8].contiguous()
    with pytest.raises(ValueError, match="min_area"):
        ops.object_moments(small, 20.0, SCALE, min_area=0)
    with pytest.raises(ValueError, match="intensity"):
        ops.sal_table(small, small, (20.0,), SCALE, intensity=[0] * 90 + [65536])
    with pytest.raises(ValueError, match="value_scale"):
        ops.object_moments(small, 20.0, 256.5)
    assert ops.object_moments(torch.zeros(1, 256, 256, device=DEV), 20.0, SCALE).sum().item() == 0


@pytest.mark.parametrize("density", [0.1, 0.41, 0.6])
@pytest.mark.parametrize("H,W", [(33, 65)] + TIERS[1:], ids=lambda v: str(v))
def test_moments_of_uniform_noise_around_the_percolation_point(H, W, density):
    field = np.stack([_ragged(S.noise(H, W, density, 11 + i), 21 + i) for i in range(2)])
    got = _check_moments(field)
    assert (got[:, 0] > 0).sum() >= 2


@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("min_area", [1, 2, 9])
def test_min_area_and_weights_on_radar_like_fields_with_planted_values(min_area, weights):
    """NaN, +-Inf, negatives and values > 1 planted; a frame per tier of the implementation"""
    for i, (H, W) in enumerate(TIERS):
        field = S.radar(2, H, W, 31 + i, plant=True)
        assert np.isnan(field).any() and np.isinf(field).any() and (field < 0).any() and (field > 1).any()
        got = _check_moments(field, min_area=min_area, intensity=WEIGHTS[weights])
        assert (got[:, 0] > 0).sum() >= 2
        if weights == "ones":
            stats = ops.object_stats(_dev(field), _dev(field), (20.0,), SCALE, min_area).cpu().numpy()
            assert (got[:, 0].sum(axis=(1, 2)) == stats[:, 0, 0, 1]).all(), "with unit weights the R of the roots add up to the area of the kept objects"
            assert ((got[:, 1] > 0).sum(axis=(1, 2)) == stats[:, 0, 0, 0]).all(), "and there is one root per kept object"


def test_moments_at_other_thresholds_and_scales():
    field = S.radar(2, 64, 64, 41, plant=True)
    every = _check_moments(field, thr=0.0)          # every pixel is an event: one object that is the frame, with the field's whole mass
    for f in range(2):
        assert every[f, :, 0, 0].tolist()[::2] == list(S.mass(S.weights(field[f], SCALE))[:2]) and (every[f, 0] > 0).sum() == 1
    assert not _check_moments(field, thr=91.0).any(), "nothing reaches 91"
    _check_moments(field, thr=35.5, scale=89.5)
    _check_moments(field, thr=1.0, scale=1.0, intensity=[7, 9])
    _check_moments(field, thr=100.0, scale=255.9, min_area=3)


# ------------------------------------------------------------------------------------------------ 2. sal_table against the yardstick
def _compare_rows(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(got[..., COUNTS] != want[..., COUNTS])
    assert bad.size == 0, f"{what}: count column differs at (frame, threshold, column of {COUNTS}) {bad[:6].tolist()}"
    dev = float(np.abs(got[..., SCORES] - want[..., SCORES]).max())
    seen[what] = max(seen.get(what, 0.0), dev)
    print(f"sal deviation, {what}: {dev:.3e}")
    assert dev <= TOL, f"{what}: a score is {dev:.3e} away from the yardstick"


def _check_table(t, p, thr=(20.0, 40.0), scale=SCALE, min_area=1, intensity=None, what=""):
    t, p = np.asarray(t, dtype=np.float32), np.asarray(p, dtype=np.float32)
    got = ops.sal_table(_dev(t), _dev(p), thr, scale, min_area, intensity)
    assert got.dtype == torch.float64 and tuple(got.shape) == (t.shape[0], len(thr), 12) and got.device.type == "cuda"
    got = got.cpu().numpy()
    _compare_rows(got, S.frame_rows(t, p, thr, scale, min_area, intensity), what)
    return got


@pytest.fixture(scope="module")
def blobs():
    return S.blobs(64, 64, 6, seed=0, margin=20)


def test_equal_shifted_smoothed_scaled_and_zero_forecasts(blobs):
    smooth = ndimage.gaussian_filter(blobs.astype(np.float64), 3).astype(np.float32)
    zero = np.zeros_like(blobs)
    t = np.stack([blobs, blobs, blobs, blobs, blobs, zero, zero])
    p = np.stack([blobs, _shift(blobs, 3, 5), smooth, np.clip(blobs * 1.3, 0, 1), zero, blobs, zero])
    got = _check_table(t, p, (20.0,), what="blobs")[:, 0]
    assert got[0].tolist() == [1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0], "pred == target: exact zeros"
    assert got[1, 1] == 0 and abs(got[1, 6]) <= 1e-12 and abs(got[1, 8]) <= 1e-12 and abs(got[1, 4] - np.hypot(3, 5) / np.hypot(64, 64)) <= 1e-12, "a shift moves L1 only"
    assert got[2, 6] > 0 and abs(got[2, 1]) < 0.05 and got[3, 1] > 0, "smoothing raises S, scaling raises A"
    assert got[4].tolist() == [1, -2, 2, 0, 0, 0, 0, 0, 0, 0, 1, 0] and got[5].tolist() == [1, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 1] and not got[6].any()


@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("H,W", [(5, 3), (33, 65)] + TIERS + SWITCHES + [(256, 256)], ids=lambda v: str(v))
def test_rows_of_radar_like_pairs(H, W, weights):
    frames = 2 if H * W > 40000 else 3
    t, p = S.radar(frames, H, W, 51, plant=True), S.radar(frames, H, W, 52, plant=True)
    p[-1] = _shift(t[-1], min(1, H - 1), min(2, W - 1))
    got = _check_table(t, p, (0.0, 20.0, 40.0, 91.0), intensity=WEIGHTS[weights], what=f"radar {H} x {W} {weights}")
    assert (got[:, 3, [5, 10, 11]] == 0).all(), "nothing reaches 91"
    if H * W >= 1000:
        assert (got[:, :, 0] == 1).all() and (got[:, 0, 5] == 1).all(), "A is defined on every frame, and S at a threshold of 0"
    assert (got[:, :, 1] == got[:, :1, 1]).all() and (got[:, :, 4] == got[:, :1, 4]).all(), "A and L1 do not depend on the threshold"
    _check_table(t, p, (20.0, 35.5), 89.5, min_area=9, what=f"radar {H} x {W} min_area 9")


@pytest.mark.parametrize("H,W", TIERS, ids=lambda v: str(v))
def test_rows_of_noise_at_41_percent(H, W):
    t = np.stack([_ragged(S.noise(H, W, 0.41, 61), 62), _ragged(S.lattice(H, W), 63)])
    p = np.stack([_ragged(S.noise(H, W, 0.41, 64), 65), _ragged(S.checkerboard(H, W), 66)])
    got = _check_table(t, p, (20.0, 60.0), what=f"noise {H} x {W}")
    assert (got[:, :, 5] == 1).all()


# ------------------------------------------------------------------------------------------------ 3. the raw entry point: sources, bitwise conditions
def _accum(pred_ptr, sample_stride, frame_stride, tgt, table, thr, T, scale=SCALE, min_area=1, intensity=None, ws=None):
    frames, H, W = tgt.shape
    nb = lib.query("adnm_valid_sal_accum_ws_bytes", frames, T, H, W, len(thr))
    assert nb >= 8 * frames * len(thr) * 12
    if ws is None:
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    lib.call("adnm_valid_sal_accum", pred_ptr, sample_stride, frame_stride, tgt.data_ptr(), table.data_ptr(), (ctypes.c_float * len(thr))(*thr), len(thr), scale,
             min_area, ops.sal_weights(intensity, scale), ws.data_ptr(), nb, frames, T, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return ws


def _table(T, nthr, tail=0):
    n = lib.query("adnm_valid_sal_block_bytes", T, nthr) // 8
    assert n == T * nthr * 12
    return torch.zeros(n + tail, dtype=torch.float64, device=DEV)


def test_a_held_frame_is_the_materialised_repeat():
    B, T, T_in, H, W, thr = 2, 3, 2, 20, 28, (20.0, 40.0)
    tn, xn = S.radar(B * T, H, W, 71), S.radar(B * T_in, H, W, 72)
    t, x = _dev(tn), _dev(xn).view(B, T_in, H, W)
    a, b = _table(T, 2), _table(T, 2)
    _accum(x.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, t, a, thr, T)          # the last input frame, held over the horizon
    held = x[:, -1:].expand(B, T, H, W).contiguous().view(B * T, H, W)
    _accum(held.data_ptr(), T * H * W, H * W, t, b, thr, T)
    assert torch.equal(_bits(a), _bits(b))
    want = S.fold(S.frame_rows(tn, held.cpu().numpy(), thr, SCALE), T)
    _compare_rows(a.cpu().numpy().reshape(T, 2, 12), want, "a held frame")
    mom = torch.empty(B * T, 4, H, W, dtype=torch.int64, device=DEV)
    lib.call("adnm_object_moments", x.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, mom.data_ptr(), 20.0, SCALE, 1, None, None, 0, B * T, T, H, W,
             torch.cuda.current_stream().cuda_stream)
    assert (mom.cpu().numpy() == S.moments(held.cpu().numpy(), 20.0, SCALE)).all()


def test_a_source_at_a_4_byte_aligned_address():
    B, T, H, W, thr = 2, 2, 17, 23, (20.0,)
    tn, pn = S.radar(B * T, H, W, 81), S.radar(B * T, H, W, 82)
    hold_p, hold_t = (torch.zeros(B * T * H * W + 1, dtype=torch.float32, device=DEV) for _ in range(2))
    off_p, off_t = hold_p[1:].view(B * T, H, W), hold_t[1:].view(B * T, H, W)
    off_p.copy_(_dev(pn)), off_t.copy_(_dev(tn))
    assert off_p.data_ptr() % 16 == 4 and off_t.data_ptr() % 16 == 4
    got = _table(T, 1)
    _accum(off_p.data_ptr(), T * H * W, H * W, off_t, got, thr, T)
    _compare_rows(got.cpu().numpy().reshape(T, 1, 12), S.fold(S.frame_rows(tn, pn, thr, SCALE), T), "a source at a 4-byte aligned address")
    assert (ops.object_moments(off_t, 20.0, SCALE).cpu().numpy() == S.moments(tn, 20.0, SCALE)).all()


@pytest.mark.parametrize("H,W", TIERS, ids=lambda v: str(v))
def test_bitwise_conditions(H, W):
    """pred IS target: exact zeros; two runs, and a second call on a zeroed table: the same bits; a call onto a table that holds a row adds
    exactly the batch sum, formed samples ascending from 0.0 (numpy float64 adds in that order)"""
    B, T, thr = 3, 2, (20.0, 40.0)
    tn, pn = S.radar(B * T, H, W, 91), S.radar(B * T, H, W, 92)
    t, p = _dev(tn), _dev(pn)
    same = _table(T, 2)
    _accum(t.data_ptr(), T * H * W, H * W, t, same, thr, T)
    same = same.cpu().numpy().reshape(T, 2, 12)
    assert (same[..., [1, 2, 4, 6, 7, 8, 9]] == 0).all() and (np.signbit(same) == 0).all(), "pred is target: exact zeros"
    assert (same[..., [0, 3]] == B).all() and (same[..., [10, 11]] == 0).all() and same[:, 0, 5].min() >= 1
    rows = ops.sal_table(t, p, thr, SCALE)
    assert torch.equal(_bits(rows), _bits(ops.sal_table(t, p, thr, SCALE))), "two runs give other bits"
    rows = rows.cpu().numpy()
    first = _table(T, 2)
    ws = _accum(p.data_ptr(), T * H * W, H * W, t, first, thr, T)
    once = first.clone()
    assert (once.cpu().numpy().reshape(T, 2, 12).view(np.int64) == S.fold(rows, T).view(np.int64)).all(), "the batch sum is not the rows added samples ascending from 0.0"
    first.zero_()
    _accum(p.data_ptr(), T * H * W, H * W, t, first, thr, T, ws=ws)
    assert torch.equal(_bits(first), _bits(once)), "a second call on a zeroed table gives other bits"
    _accum(t.data_ptr(), T * H * W, H * W, p, first, thr, T, ws=ws)          # the fields swapped: another batch onto a table that holds a row
    swapped = ops.sal_table(p, t, thr, SCALE).cpu().numpy()
    want = S.fold(swapped, T, onto=once.cpu().numpy().reshape(T, 2, 12))
    assert (first.cpu().numpy().reshape(T, 2, 12).view(np.int64) == want.view(np.int64)).all(), "a second batch does not add exactly its batch sum"


def test_more_items_than_workgroups_in_the_workspace_routes():
    """130 x 129 frames keep their records in the workspace, which has 256 slices: 66 frames at 4 thresholds make 264 items, so eight
    workgroups work a second item in their slice"""
    frames, H, W, thr = 66, 130, 129, (10.0, 20.0, 30.0, 40.0)
    one = S.radar(3, H, W, 101)
    t, p = np.zeros((frames, H, W), dtype=np.float32), np.zeros((frames, H, W), dtype=np.float32)
    t[0], t[1], t[64], t[65] = one[0], one[1], one[1], _ragged(S.checkerboard(H, W), 5)
    p[0], p[1], p[64], p[65] = one[1], one[2], one[2], one[0]
    got = ops.sal_table(_dev(t), _dev(p), thr, SCALE).cpu().numpy()
    pick = [0, 1, 64, 65]
    _compare_rows(got[pick], S.frame_rows(t[pick], p[pick], thr, SCALE), "264 items on 256 slices")
    assert not got[2:64].any()
    mom = ops.object_moments(_dev(np.concatenate([t] * 4)), 20.0, SCALE).cpu().numpy()          # 264 frames
    assert (mom[[0, 65, 66 + 64, 3 * 66 + 65]] == S.moments(t[[0, 65, 64, 65]], 20.0, SCALE)).all() and not mom[2:64].any()


# ------------------------------------------------------------------------------------------------ 4. the workspace and output contracts
@pytest.mark.parametrize("H,W", TIERS, ids=lambda v: str(v))
def test_guarded_and_poisoned_workspaces(monkeypatch, H, W):
    """every workspace between poisoned guards and itself poisoned: the guards stay, the results are bit for bit those of a plain run"""
    thr = (20.0, 40.0)
    tn, pn = S.radar(3, H, W, 111, plant=True), S.radar(3, H, W, 112, plant=True)
    t, p = _dev(tn), _dev(pn)
    plain = ops.sal_table(t, p, thr, SCALE, 2, TOP), ops.object_moments(t, 20.0, SCALE, 2, TOP)
    with guarded_workspaces(monkeypatch) as g:
        guarded = ops.sal_table(t, p, thr, SCALE, 2, TOP), ops.object_moments(t, 20.0, SCALE, 2, TOP)
        g.check()
        assert g.calls == (1 if H * W <= 114 * 116 else 2), "the item rows always; the moments' slices from the second tier on"
        sizes = sorted(r[2] for r in g.records)
        assert sizes[-1] == lib.query("adnm_valid_sal_accum_ws_bytes", 3, 3, H, W, 2) and sizes[0] in (sizes[-1], lib.query("adnm_object_moments_ws_bytes", 3, 3, H, W))
    assert torch.equal(_bits(plain[0]), _bits(guarded[0])) and torch.equal(plain[1], guarded[1]), "a result depends on what a workspace held"
    _compare_rows(guarded[0].cpu().numpy(), S.frame_rows(tn, pn, thr, SCALE, 2, TOP), f"poisoned workspace {H} x {W}")


@pytest.mark.parametrize("H,W", TIERS, ids=lambda v: str(v))
def test_outputs_filled_with_both_patterns(monkeypatch, H, W):
    """torch.empty hands out pattern-filled tensors: no element of the moments image keeps its pattern, and the item rows the fold reads were
    all written (a row left alone would reach the table as a payload NaN)"""
    thr = (20.0, 91.0)
    tn, pn = S.radar(2, H, W, 121), S.radar(2, H, W, 122)
    tn[1] = 0          # an empty frame: its rows and its moments are written all the same
    t, p = _dev(tn), _dev(pn)
    runs, records = [], []
    for pattern in (0, 1):
        with poisoned_outputs(monkeypatch, pattern) as po:
            with guarded_workspaces(monkeypatch) as g:          # the workspace arrives poisoned too
                runs.append((ops.sal_table(t, p, thr, SCALE), ops.object_moments(t, 20.0, SCALE)))
                g.check()
            records.append(po.records)
    assert unwritten(records[0], records[1]) == {}, "an output element nobody wrote"
    assert any(r[2] == "out" and r[0].dtype == torch.int64 for r in records[0]), "the moments image was not among the allocations"
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1])
    assert bool(torch.isfinite(runs[0][0]).all()), "a workspace row that was never written reached the table"
    assert (runs[0][1].cpu().numpy() == S.moments(tn, 20.0, SCALE)).all()
    _compare_rows(runs[0][0].cpu().numpy(), S.frame_rows(tn, pn, thr, SCALE), f"poisoned outputs {H} x {W}")


# ------------------------------------------------------------------------------------------------ 5. the Validator end to end
class Drift(torch.nn.Module):
    """a stand-in forecast: the last input frame, moved one more pixel to the right and weakened with every lead"""
    def forward(self, x):
        last = x[:, -1, 0].float()
        return torch.stack([torch.roll(last, t + 1, dims=-1) * (1.0 - 0.15 * t) for t in range(3)], dim=1)


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


@pytest.mark.parametrize("size", [32, 64])
def test_validator_with_sal_end_to_end(size):
    from adnm_hip.validate import Validator, sal_doubles, sal_entries
    from models.loss import RainfallLoss
    B, T, H, W, thr = 2, 3, size, size, [20, 30.5]
    spec = dict(min_area=2, intensity=TOP)
    seq = S.radar(2 * B * 5, H, W, 131).reshape(2, B, 5, 1, H, W) * 0.7
    data = [(_dev(seq[i, :, :2]), _dev(seq[i, :, 2:])) for i in range(2)]
    kw = dict(pools=(4,), persistence=True, joint=True, objects=2)
    val = Validator(Drift(), RainfallLoss(), T, SCALE, thr, sal=spec, **kw)
    former = Validator(Drift(), RainfallLoss(), T, SCALE, thr, sal=None, **kw)
    alone = Validator(Drift(), RainfallLoss(), T, SCALE, thr, sal=spec)
    try:
        n = sal_doubles(T, len(thr), spec)
        assert n == T * len(thr) * 12
        want, batches = np.zeros((T, len(thr), 12)), []
        for x, tgt in data:            # two steps through the captured graph: the second batch is added as its own batch sum
            out = val.step(x, tgt)
            rows = ops.sal_table(tgt.view(B * T, H, W), out.view(B * T, H, W).contiguous(), thr, SCALE, 2, TOP).cpu().numpy()
            _compare_rows(rows, S.frame_rows(tgt.cpu().numpy().reshape(B * T, H, W), out.cpu().numpy().reshape(B * T, H, W), thr, SCALE, 2, TOP), f"validator {size}")
            want = S.fold(rows, T, onto=want)
            batches.append(S.fold(rows, T))
            former.step(x, tgt)
            alone.step(x, tgt)
        assert want[:, 0, 5].min() > 0 and np.abs(want[:, 0, 6]).min() > 0, "no objects, or a forecast equal to the target: nothing is tested"
        assert val._block.numel() == former._block.numel() + n and former.sal is None
        assert all(e.get("ws_sal") is None for e in former._fwd._graphs.values())
        got = val._block[-n:].cpu().numpy().reshape(T, len(thr), 12)
        assert (got.view(np.int64) == want.view(np.int64)).all(), "the table at the end of the one allocation is not the op's rows folded batch by batch"
        assert torch.equal(_bits(val._block[:-n]), _bits(former._block)), "a former offset moved, or a former pass counts differently"
        assert torch.equal(_bits(alone._block[-n:]), _bits(val._block[-n:])), "the SAL table depends on the other options"
        res, old = val.done(per_lead=True), former.done(per_lead=True)
        assert "sal" not in old and "sal" not in old["per_lead"]
        assert list(res) == list(old)[:-1] + ["sal", "per_lead"] and list(res["per_lead"]) == list(old["per_lead"]) + ["sal"]
        assert _same_tree({k: res[k] for k in old if k != "per_lead"}, {k: old[k] for k in old if k != "per_lead"}), "a former entry moved"
        assert _same_tree({k: res["per_lead"][k] for k in old["per_lead"]}, old["per_lead"]), "a former per-lead entry moved"
        assert _same_tree(res["sal"], sal_entries(want.sum(axis=0), thr, (2, tuple(TOP)))) and _same_tree(res["per_lead"]["sal"], sal_entries(want, thr, (2, tuple(TOP))))
        assert res["sal"]["min_area"] == 2 and res["sal"][20]["frames_A"] == 2 * B * T
        print(f"sal end to end at {size}, threshold 20:", {k: v for k, v in res["sal"][20].items()})
        # a second epoch holds the second batch alone: it does not depend on the first
        val.reset()
        val.step(*data[1])
        assert (val._block[-n:].cpu().numpy().reshape(T, len(thr), 12).view(np.int64) == batches[1].view(np.int64)).all(), "a batch depends on the one before"
        # once the graph exists a step allocates nothing
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        val.step(*data[0])
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        val.reset()
        assert float(val._block.abs().sum()) == 0.0, "reset() zeroes the tail"
    finally:
        val.close()
        former.close()
        alone.close()


def test_validator_raises_at_the_first_step_on_a_frame_above_the_limit():
    from adnm_hip.validate import Validator
    from models.loss import RainfallLoss

    class Last(torch.nn.Module):
        def forward(self, x):
            return x[:, -1:, 0].float()
    val = Validator(Last(), RainfallLoss(), 1, SCALE, [20], ssim=False, sal=True)
    try:
        x = torch.zeros(1, 1, 1, 257, 256, device=DEV)
        with pytest.raises(RuntimeError, match="65536"):
            val.step(x, x.clone())
    finally:
        val.close()
