"""Radially averaged power spectra without a GPU: ops.spectrum_bins against the yardstick's bin image, the yardstick against Parseval,
validate.aggregate on a hand-made spectrum table, the arguments, and the three entry points at the C boundary (declared, exported,
refusing every limit before any launch)."""
import ctypes

import numpy as np
import pytest

import spectrum_ref as S
from adnm_hip import lib, ops

NEW = ("adnm_valid_spectrum_block_bytes", "adnm_valid_spectrum_accum_ws_bytes", "adnm_valid_spectrum_accum")
SIZES = [(8, 8), (16, 64), (64, 16), (128, 128), (512, 8)]


# ------------------------------------------------------------------------------------------------ the bins
@pytest.mark.parametrize("H,W", SIZES)
def test_spectrum_bins_equal_the_mask_counts_and_every_coefficient_is_counted_once(H, W):
    n_r, wavelength = ops.spectrum_bins(H, W)
    want, corners = S.bin_counts(H, W)
    L = max(H, W)
    assert n_r.shape == wavelength.shape == (L // 2,) and n_r.dtype == np.int64 and wavelength.dtype == np.float64
    assert (n_r == want).all()
    assert n_r[0] == 1 and corners > 0 and int(n_r.sum()) + corners == H * W
    assert np.isinf(wavelength[0]) and (wavelength[1:] == L / np.arange(1, L // 2)).all()


def test_the_bin_follows_the_longer_side():
    """(16, 64): ky is scaled by L/H = 4, so (ky, kx) = (1, 0) lies in bin 4 and (0, 1) in bin 1"""
    img = S.bin_image(16, 64)
    assert img[1, 0] == 4 and img[0, 1] == 1 and img[15, 0] == 4 and img[8, 0] == 32 and img[0, 32] == 32
    n_r, _ = ops.spectrum_bins(16, 64)
    assert n_r[1] == 2 and n_r[4] == (img == 4).sum()


@pytest.mark.parametrize("bad", [(96, 96), (4, 8), (8, 1024), (0, 8), (64, 48), (-8, 8), (8.0, 8), (True, 8)])
def test_spectrum_bins_refuses(bad):
    with pytest.raises(ValueError, match="spectrum"):
        ops.spectrum_bins(*bad)


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("case", S.CASES[:4], ids=S.case_id)
def test_parseval_on_the_yardstick(case):
    t, p = S.fields(*case)
    assert (t < 0).any() and (t > 1).any() and (p < 0).any() and (p > 1).any(), "the clip is not exercised"
    sums, corners = S.ref_sums(t, p, S.SCALE, corners=True)
    o, f = S.clipped(t, S.SCALE), S.clipped(p, S.SCALE)
    for col, want in ((0, (o * o).sum(axis=(1, 2))), (1, (f * f).sum(axis=(1, 2))), (2, (o * f).sum(axis=(1, 2)))):
        got = sums[:, :, col].sum(axis=1) + corners[:, col]
        assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), col
    assert sums.shape == (case[0], max(case[1:3]) // 2, 3) and (sums[..., :2] > 0).all()
    # Cauchy-Schwarz per bin, and the float32 restatement is close but not equal
    assert (np.abs(sums[..., 2]) <= np.sqrt(sums[..., 0] * sums[..., 1]) * (1 + 1e-12)).all()
    rel, _ = S.deviation(S.ref_sums_f32(t, p, S.SCALE), sums)
    assert 0 < rel < 1e-3


def test_a_nan_stays_a_nan_in_the_yardstick():
    t, p = (a.copy() for a in S.fields(*S.CASES[0]))
    t[0, 3, 3] = np.nan
    sums = S.ref_sums(t, p, S.SCALE)
    assert np.isnan(sums[0, :, 0]).all() and np.isnan(sums[0, :, 2]).all() and np.isfinite(sums[0, :, 1]).all() and np.isfinite(sums[1]).all()


# ------------------------------------------------------------------------------------------------ aggregate
T, THR, H, W = 3, [20, 30, 35, 40], 16, 64
R = 32


def _hand_block(seed, extra=0):
    """header, main table, `extra` doubles of other tables, then a spectrum table with C <= sqrt(P_o P_f)"""
    from adnm_hip.validate import block_doubles, spectrum_doubles
    rng = np.random.default_rng(seed)
    n = len(THR)
    main = rng.integers(1, 1 << 20, (T, 4 * n + 3)).astype(np.float64)
    main[:, 4 * n:] += rng.random((T, 3))
    tab = rng.random((T, R, 3)) * 1000.0 + 1.0
    tab[..., 2] = np.sqrt(tab[..., 0] * tab[..., 1]) * (2 * rng.random((T, R)) - 1)
    blk = np.concatenate([[1.25, 2, 6, 0], main.ravel(), rng.integers(0, 1 << 20, extra).astype(np.float64), tab.ravel()])
    assert blk.shape == (block_doubles(T, n)[0] + extra + spectrum_doubles(T, (H, W)),) and spectrum_doubles(T, (H, W)) == T * R * 3
    return blk, tab


def _same(a, b):
    return repr(a) == repr(b)


def test_aggregate_with_a_spectrum_table():
    from adnm_hip.validate import aggregate
    hw, n = H * W, len(THR)
    blk, tab = _hand_block(1)
    tab[:, :, 1] = tab[:, :, 0] * 0.9                  # the forecast keeps 90 % of the power ...
    tab[:, 11:, 1] = tab[:, 11:, 0] * 0.25             # ... down to bin 10, and a quarter below
    tab[:, 20, 1] = tab[:, 20, 0] * 2.0                # a later bin above one half does not count: every bin up to r
    tab[1, 7, 1] = tab[1, 7, 0] * 0.1                  # frame index 1 alone fails at bin 7 already
    tab[2, 1, 1] = tab[2, 1, 0] * 0.4                  # frame index 2 fails at bin 1
    tab[2, 5, :2] = 0.0                                # an empty bin: coherence NaN there
    blk[-tab.size:] = tab.ravel()
    res = aggregate(blk, THR, T, hw, None, per_lead=True, spectrum=(H, W))
    plain = aggregate(blk[:4 + T * (4 * n + 3)], THR, T, hw, None, per_lead=True)
    assert set(res) == set(plain) | {"spectrum"} and set(res["per_lead"]) == set(plain["per_lead"]) | {"spectrum"}
    assert _same({k: res[k] for k in plain if k != "per_lead"}, {k: plain[k] for k in plain if k != "per_lead"})
    assert _same({k: res["per_lead"][k] for k in plain["per_lead"]}, plain["per_lead"])
    sp, lead = res["spectrum"], res["per_lead"]["spectrum"]
    keys = ["wavenumber", "wavelength_px", "target", "forecast", "ratio", "coherence", "effective_resolution_px"]
    assert list(sp) == keys == list(lead)
    n_r, wavelength = ops.spectrum_bins(H, W)
    samples = 6.0
    tot = tab.sum(axis=0)
    assert (sp["wavenumber"] == np.arange(R)).all() and (sp["wavelength_px"] == wavelength).all()
    assert np.allclose(sp["target"], tot[:, 0] / (n_r * samples * T), rtol=1e-15) and np.allclose(sp["forecast"], tot[:, 1] / (n_r * samples * T), rtol=1e-15)
    assert np.allclose(sp["ratio"], tot[:, 1] / tot[:, 0], rtol=1e-15)
    assert np.allclose(sp["coherence"], tot[:, 2] / np.sqrt(tot[:, 0] * tot[:, 1]), rtol=1e-15)
    # over the horizon the SUMS decide: rows 1 and 2 fail early on their own, the sum of the three rows need not
    keep = int(np.cumprod(tot[1:, 1] / tot[1:, 0] >= 0.5).sum())
    assert keep in (0, 6, 10) and isinstance(sp["effective_resolution_px"], float)
    assert sp["effective_resolution_px"] == (64.0 / keep if keep else float("inf"))
    for k in ("target", "forecast", "ratio", "coherence"):
        assert lead[k].shape == (T, R), k
    assert np.allclose(lead["target"], tab[:, :, 0] / (n_r * samples), rtol=1e-15) and np.allclose(lead["forecast"][:2], tab[:2, :, 1] / (n_r * samples), rtol=1e-15)
    assert lead["effective_resolution_px"].shape == (T,)
    assert lead["effective_resolution_px"][0] == 64.0 / 10 and lead["effective_resolution_px"][1] == 64.0 / 6 and np.isinf(lead["effective_resolution_px"][2])
    assert np.isnan(lead["coherence"][2, 5]) and np.isfinite(np.delete(lead["coherence"][2], 5)).all() and np.isfinite(sp["coherence"]).all()
    short = aggregate(blk, THR, T, hw, None, spectrum=(H, W))
    assert "per_lead" not in short and _same(short["spectrum"], sp)


def test_effective_resolution_is_inf_when_bin_one_fails_and_the_last_bin_when_none_does():
    from adnm_hip.validate import aggregate
    blk, tab = _hand_block(2)
    tab[:, :, 1] = tab[:, :, 0]
    blk[-tab.size:] = tab.ravel()
    assert aggregate(blk, THR, T, H * W, None, spectrum=(H, W))["spectrum"]["effective_resolution_px"] == 64.0 / 31
    tab[:, 1, 1] = tab[:, 1, 0] * 0.49
    blk[-tab.size:] = tab.ravel()
    assert aggregate(blk, THR, T, H * W, None, spectrum=(H, W))["spectrum"]["effective_resolution_px"] == float("inf")
    tab[:, 1, 1] = tab[:, 1, 0] * 0.5                      # exactly one half keeps the bin
    tab[:, 2, 1] = np.nan                                  # a NaN fails it
    blk[-tab.size:] = tab.ravel()
    assert aggregate(blk, THR, T, H * W, None, spectrum=(H, W))["spectrum"]["effective_resolution_px"] == 64.0


def test_the_table_is_last_and_a_block_without_it_aggregates_as_before():
    from adnm_hip.validate import aggregate, block_doubles, fss_doubles
    n, fss = len(THR), (1, 5)
    extra = sum(fss_doubles(T, n, fss))
    blk, tab = _hand_block(3, extra=extra)
    res = aggregate(blk, THR, T, H * W, None, fss=fss, per_lead=True, spectrum=(H, W))
    former = aggregate(blk[:-tab.size], THR, T, H * W, None, fss=fss, per_lead=True)
    assert list(res) == list(former)[:-1] + ["spectrum", "per_lead"] and list(res["per_lead"]) == list(former["per_lead"]) + ["spectrum"]
    assert _same({k: res[k] for k in former if k != "per_lead"}, {k: former[k] for k in former if k != "per_lead"})
    assert _same({k: res["per_lead"][k] for k in former["per_lead"]}, former["per_lead"])
    alone = aggregate(np.concatenate([blk[:block_doubles(T, n)[0]], tab.ravel()]), THR, T, H * W, None, per_lead=True, spectrum=(H, W))
    assert _same(alone["spectrum"], res["spectrum"]) and _same(alone["per_lead"]["spectrum"], res["per_lead"]["spectrum"])
    plain = aggregate(blk[:block_doubles(T, n)[0]], THR, T, H * W, None)
    assert list(plain) == ["threshold_metrics", "FAR", "RMSE", "MAE", "MSE", "SSIM", "LPIPS", "loss_sum", "loss_mean", "batches", "samples", "nonfinite"]
    with pytest.raises(ValueError, match="doubles"):
        aggregate(blk, THR, T, H * W, None, fss=fss)                               # the table is there, the argument is not
    with pytest.raises(ValueError, match="spectrum"):
        aggregate(blk, THR, T, H * W, None, fss=fss, spectrum=(H, 2 * W))          # another frame size, another table
    with pytest.raises(ValueError, match="spectrum"):
        aggregate(blk, THR, T, 96 * 96, None, fss=fss, spectrum=(96, 96))


# ------------------------------------------------------------------------------------------------ the arguments
def test_validator_arguments_and_doubles():
    import inspect

    import torch
    from adnm_hip.validate import Validator, spectrum_doubles
    from models.loss import enRainfallLoss
    assert inspect.signature(Validator.__init__).parameters["spectrum"].default is False
    assert spectrum_doubles(20) == spectrum_doubles(20, None) == spectrum_doubles(20, False) == 0
    assert spectrum_doubles(20, (128, 128)) == 20 * 64 * 3 and spectrum_doubles(5, (16, 64)) == spectrum_doubles(5, (64, 16)) == 5 * 32 * 3
    model, crit = torch.nn.Identity(), enRainfallLoss()
    assert Validator(model, crit, 20, 255.0).spectrum is False and Validator(model, crit, 20, 255.0, spectrum=True).spectrum is True


def test_power_spectrum_refuses_what_is_not_two_gpu_tensors():
    import torch
    a = torch.zeros(2, 8, 8)
    with pytest.raises(RuntimeError):
        ops.power_spectrum(a, a, 255.0)                    # CPU tensors
    with pytest.raises(RuntimeError):
        ops.power_spectrum(a.numpy(), a.numpy(), 255.0)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_new_prototypes_are_declared_and_exported():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_valid_spectrum_block_bytes"] == ("int64_t", ["int64_t"] * 3)
    assert protos["adnm_valid_spectrum_accum_ws_bytes"] == ("int64_t", ["int64_t"] * 4)
    assert protos["adnm_valid_spectrum_accum"] == ("int", ["const float*", "int64_t", "int64_t", "const float*", "void*", "float", "void*", "int64_t", "int64_t",
                                                           "int64_t", "int64_t", "int64_t", "adnm_stream_t"])


def test_byte_queries():
    q = lib.query
    blk, ws = "adnm_valid_spectrum_block_bytes", "adnm_valid_spectrum_accum_ws_bytes"
    assert q(blk, 20, 128, 128) == 8 * 20 * 64 * 3 and q(blk, 1, 16, 64) == q(blk, 1, 64, 16) == 8 * 32 * 3 and q(blk, 3, 512, 8) == 8 * 3 * 256 * 3
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 4, 8), (1, 8, 4), (1, 1024, 8), (1, 8, 1024), (1, 96, 96), (1, 48, 64), (1, 64, 24), (1, 0, 8), (1, -8, 8)):
        assert q(blk, *bad) == -1, bad
    # per frame and kx = 0 .. W/2: two complex columns of H for the column pass, R x 3 float partial sums for the fold
    assert q(ws, 40, 20, 128, 128) == 40 * 65 * (2 * 128 * 8 + 64 * 3 * 4)
    assert q(ws, 2, 2, 16, 64) == 2 * 33 * (2 * 16 * 8 + 32 * 3 * 4) and q(ws, 2, 1, 64, 16) == 2 * 9 * (2 * 64 * 8 + 32 * 3 * 4)
    assert q(ws, 65535, 1, 8, 8) > 0
    assert q(ws, 80, 7, 128, 128) == -1, "T does not divide frames"
    assert q(ws, 80, 0, 128, 128) == -1 and q(ws, 80, -1, 128, 128) == -1, "T < 1"
    assert q(ws, 0, 1, 128, 128) == -1, "no frame"
    assert q(ws, 65536, 1, 8, 8) == -1, "frames > 65535"
    for H_, W_ in ((96, 96), (4, 8), (8, 4), (1024, 8), (8, 1024), (0, 8), (8, 0), (48, 64), (64, 100), (-64, 64)):
        assert q(ws, 4, 2, H_, W_) == -1, (H_, W_)


def test_every_limit_is_refused_on_the_host_with_its_own_message():
    """fake addresses: anything that reached a launch would fault, and the stream is never touched"""
    so = lib.load()

    def call(pred=16, ss=20 * 64 * 64, fs=64 * 64, tgt=32, table=64, ws=128, ws_bytes=1 << 40, frames=40, T=20, H_=64, W_=64):
        rc = so.adnm_valid_spectrum_accum(pred, ss, fs, tgt, table, 90.0, ws, ws_bytes, frames, T, H_, W_, None)
        return rc, lib.last_error()

    cases = [(dict(pred=None), "null pointer"), (dict(tgt=None), "null pointer"), (dict(table=None), "null pointer"), (dict(ws=None), "null pointer"),
             (dict(pred=18), "4-byte aligned"), (dict(tgt=34), "4-byte aligned"), (dict(table=68), "table must be 8-byte aligned"),
             (dict(ws=132), "workspace must be 8-byte aligned"),
             (dict(H_=96), "powers of two in 8..512"), (dict(W_=4), "powers of two in 8..512"), (dict(H_=1024), "powers of two in 8..512"),
             (dict(W_=0), "powers of two in 8..512"), (dict(H_=48, W_=48, fs=48 * 48), "powers of two in 8..512"),
             (dict(T=0), "must divide frames"), (dict(T=7), "must divide frames"), (dict(frames=0), "must divide frames"),
             (dict(frames=65540, T=20), "frames <= 65535"),
             (dict(fs=64 * 64 - 1), "pred_frame_stride"), (dict(fs=-4096), "pred_frame_stride"),
             (dict(ss=-1), "pred_sample_stride"),
             (dict(ws_bytes=lib.query("adnm_valid_spectrum_accum_ws_bytes", 40, 20, 64, 64) - 1), "workspace")]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == -1 and text in err and "valid_spectrum_accum" in err, (kw, rc, err)
    assert len({text for _, text in cases}) == 10, "one message per limit"
