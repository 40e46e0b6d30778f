"""The forecast-rendering feature without a GPU: the numpy restatement of the value rule (tests/forecast_ref.py) against matplotlib's
own output (tests/golden/forecast_render_*.npz, tools/make_golden_forecast.py), the Palette value type, the PNG writer, and the new
entry point at the C boundary (declared, exported, additive, refusing bad arguments before any launch)."""
import ctypes
import os

import numpy as np
import pytest

import forecast_ref as R
from adnm_hip import lib


# ------------------------------------------------------------------------------------------------ 1. the restatement is matplotlib's
@pytest.mark.parametrize("name", ["shanghai", "laps"])
def test_restatement_reproduces_the_fixture(name):
    z = R.load_fixture(name)
    edges, rgba = R.load_palette(name)
    B, T, H, W = z["pred"].shape
    assert z["pred"].dtype == np.float32 and (B, T, H, W) == ((2, 20, 16, 12) if name == "shanghai" else (2, 3, 16, 12))
    assert (float(z["pixel_scale"]), int(z["frame_start"]), int(z["frame_step"]), int(z["gap"])) == ((90.0, 1, 2, 10) if name == "shanghai" else (0.0, 0, 1, 10))
    fields, strip = R.render(z["pred"], edges, rgba, float(z["pixel_scale"]), int(z["frame_start"]), int(z["frame_step"]), int(z["gap"]))
    assert z["fields"].dtype == np.uint8 and z["fields"].shape == (B, T, H, W)
    n = 10 if name == "shanghai" else 3
    assert z["strip"].dtype == np.uint8 and z["strip"].shape == (B, H, n * W + (n - 1) * 10, 4)
    assert np.array_equal(fields, z["fields"]), f"{int((fields != z['fields']).sum())} field bytes differ"
    assert np.array_equal(strip, z["strip"]), f"{int((strip != z['strip']).any(-1).sum())} strip pixels differ"
    # the fixture exercises the table: every colour but at most a few is hit, and the gap is there
    assert len({tuple(c) for c in z["strip"].reshape(-1, 4)}) >= len(rgba) - 2
    assert (z["strip"][:, :, W:W + 10] == 255).all()


def test_fixture_holds_the_planted_cases():
    z = R.load_fixture("shanghai")
    p = z["pred"].reshape(-1)
    prod = p * np.float32(90.0)
    assert p.min() >= 0.0 and prod.max() < 256.0, "the fixture stays inside the uint8 range"
    below = sum(bool((prod == np.nextafter(np.float32(m), np.float32(0))).any()) for m in range(1, 90))
    assert below >= 60, f"only {below} products one ulp below an integer"
    for e in R.load_palette("shanghai")[0]:
        assert (p == np.float32(e / 90.0)).any(), e
    z = R.load_fixture("laps")
    p = z["pred"].reshape(-1)
    for e in R.load_palette("laps")[0]:
        f = np.float32(e)
        for v in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
            assert (p == v).any(), (e, v)


# ------------------------------------------------------------------------------------------------ 2. Palette
def test_palette_round_trips_and_rounds_edges_up(tmp_path):
    from adnm_hip.forecast import Palette
    down = 0
    for name in ("shanghai", "laps"):
        edges, rgba = R.load_palette(name)
        pal = Palette.load(os.path.join(R.GOLDEN, f"forecast_palette_{name}.json"))
        assert pal.nbins == len(rgba) and pal.edges == tuple(edges) and np.array_equal(pal.colours, rgba) and pal.colours.dtype == np.uint8
        assert pal.bounds.dtype == np.float32 and pal.bounds.shape == (len(edges),)
        for k, e in enumerate(edges):
            assert np.float64(pal.bounds[k]) >= e, (name, k)
            assert np.float64(np.nextafter(pal.bounds[k], np.float32(-np.inf))) < e, (name, k)
            down += bool(np.float64(np.float32(e)) < e)
        again = Palette.from_json(pal.to_json())
        assert again == pal and np.array_equal(again.bounds, pal.bounds)
        pal.save(str(tmp_path / "p.json"))
        assert open(tmp_path / "p.json").read() == open(os.path.join(R.GOLDEN, f"forecast_palette_{name}.json")).read()
    assert down >= 3, "no LAPS edge rounds down to float32: the round-up is not tested"
    # float colours: (c * 255).astype(uint8), as matplotlib converts them
    edges, rgba = R.load_palette("shanghai")
    assert np.array_equal(Palette(edges, rgba / 255).colours, rgba)
    with pytest.raises(ValueError):
        Palette(list(range(34)), np.zeros((33, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        Palette([0, 1, 2], np.zeros((3, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        Palette([0, 2, 1], np.zeros((2, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        Palette([0, 1], np.full((1, 4), 1.5))


# ------------------------------------------------------------------------------------------------ 3. save_png
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (7, 1), (16, 210), (128, 1370)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_save_png_decodes_to_the_same_bytes(tmp_path, hw):
    from adnm_hip.forecast import save_png
    img = np.random.default_rng(hw[0] * 1000 + hw[1]).integers(0, 256, size=hw + (4,), dtype=np.uint8)
    path = str(tmp_path / "a.png")
    save_png(path, img)
    got = R.decode_png(path)
    assert got.shape == img.shape and np.array_equal(got, img)
    with pytest.raises(ValueError):
        save_png(path, img[..., :3])
    with pytest.raises(ValueError):
        save_png(path, img.astype(np.float32))


def test_save_png_of_the_fixture_strip_is_the_reference_picture(tmp_path):
    from adnm_hip.forecast import save_png
    strip = R.load_fixture("shanghai")["strip"]
    save_png(str(tmp_path / "s.png"), strip[1])
    assert np.array_equal(R.decode_png(str(tmp_path / "s.png")), strip[1])


# ------------------------------------------------------------------------------------------------ 4. the C boundary
def test_entry_point_is_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    assert "adnm_forecast_render" in protos, "adnm_forecast_render is not declared in include/adnm_hip.h"
    ret, args = protos["adnm_forecast_render"]
    assert ret == "int" and args[-1] == "adnm_stream_t" and len(args) == 15
    assert args[:6] == ["const float*", "uint8_t*", "uint8_t*", "const float*", "const uint8_t*", "int64_t"]
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), "adnm_forecast_render"), "declared but not exported"
    assert lib.load().adnm_abi_version() == 11


# ------------------------------------------------------------------------------------------------ 5. refusals before any launch
def test_arguments_are_checked_on_the_host():
    so = lib.load()
    edges = (ctypes.c_float * 34)(*range(34))
    down = (ctypes.c_float * 5)(0, 5, 10, 9, 20)
    pal = (ctypes.c_uint8 * (4 * 33))()
    P = 64   # a dummy, aligned, never dereferenced "device pointer": every call below is refused before a launch

    def call(pred=P, fields=P, strip=P, b=edges, c=pal, nbins=16, scale=90.0, B=2, T=20, H=16, W=12, start=1, step=2, gap=10):
        return so.adnm_forecast_render(pred, fields, strip, b, c, nbins, scale, B, T, H, W, start, step, gap, None)

    for kw, text in (({"nbins": 0}, "1..32 bins"), ({"nbins": 33}, "1..32 bins"), ({"b": down, "nbins": 4}, "ascending"),
                     ({"start": 20}, "frame_start"), ({"start": 25}, "frame_start"), ({"start": -1}, "frame_start"), ({"step": 0}, "frame_step"),
                     ({"fields": None, "strip": None}, "no output"), ({"pred": None}, "null pointer"), ({"b": None}, "null pointer"),
                     ({"c": None}, "null pointer"), ({"gap": -1}, "gap"), ({"scale": -1.0}, "pixel_scale"), ({"scale": float("nan")}, "pixel_scale"),
                     ({"B": 0}, "bad shape"), ({"B": 1 << 12, "T": 1 << 10, "H": 1 << 5, "W": 1 << 4}, "bad shape"),
                     ({"T": 1 << 20, "H": 1, "W": 32, "B": 1, "step": 1, "start": 0}, "pixels wide"), ({"strip": 66}, "aligned")):
        assert call(**kw) == -1, kw
        assert text in lib.last_error(), (kw, lib.last_error())
