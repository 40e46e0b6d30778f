"""A numpy restatement of adnm_forecast_render's value rule (include/adnm_hip.h), for the forecast tests only.  It compares the way
matplotlib does — the fp32 value, widened, against the DOUBLE edges — so it shares neither the kernel's fp32 comparison nor the
package's rounding of the edges; tests/test_forecast_host.py pins it to matplotlib's own output (tests/golden/forecast_render_*.npz)."""
import json
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_palette(name):
    """-> (edges as doubles, (K, 4) uint8 RGBA rows) of tests/golden/forecast_palette_<name>.json"""
    with open(os.path.join(GOLDEN, f"forecast_palette_{name}.json")) as f:
        d = json.load(f)
    return [float(e) for e in d["bounds"]], np.asarray(d["rgba"], dtype=np.uint8)


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, f"forecast_render_{name}.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def strip_width(T, W, frame_start, frame_step, gap):
    n = len(range(frame_start, T, frame_step))
    return n * W + (n - 1) * gap


def render(pred, edges, rgba, pixel_scale, frame_start=0, frame_step=1, gap=10):
    """pred (B, T, H, W) fp32 -> (fields (B, T, H, W) uint8, strip (B, H, Ws, 4) uint8)"""
    p = np.asarray(pred, dtype=np.float32)
    assert p.ndim == 4
    B, T, H, W = p.shape
    e = np.asarray(edges, dtype=np.float64)
    rgba = np.asarray(rgba, dtype=np.uint8)
    K = rgba.shape[0]
    assert e.shape == (K + 1,) and (np.diff(e) > 0).all()
    bad = np.zeros(p.shape, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        if pixel_scale:
            prod = p * np.float32(pixel_scale)                   # the fp32 product
            c = np.where(np.isnan(prod), np.float32(0), np.clip(prod, np.float32(0), np.float32(255)))
            fields = np.trunc(c).astype(np.uint8)
            v = fields.astype(np.float64)
        else:
            bad = np.isnan(p)
            v = np.where(bad, 0.0, p.astype(np.float64))
    idx = np.clip(np.searchsorted(e, v, side="right") - 1, 0, K - 1)   # (number of edges <= v) - 1
    colour = rgba[idx]
    if not pixel_scale:
        idx[bad] = 0
        colour[bad] = 0
        fields = idx.astype(np.uint8)
    sel = list(range(frame_start, T, frame_step))
    strip = np.full((B, H, strip_width(T, W, frame_start, frame_step, gap), 4), 255, dtype=np.uint8)
    for j, t in enumerate(sel):
        x = j * (W + gap)
        strip[:, :, x:x + W] = colour[:, t]
    return fields, strip


def decode_png(path):
    """an 8-bit RGBA PNG -> (H, W, 4) uint8, with PIL where importable, otherwise by hand (unfiltered scanlines only)"""
    try:
        from PIL import Image
        img = Image.open(path)
        assert img.mode == "RGBA"
        return np.asarray(img, dtype=np.uint8)
    except ImportError:
        data = open(path, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        pos, idat, W, H = 8, b"", None, None
        while pos < len(data):
            n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
            body = data[pos + 8:pos + 8 + n]
            assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
            if tag == b"IHDR":
                W, H, depth, ctype, comp, filt, inter = struct.unpack(">IIBBBBB", body)
                assert (depth, ctype, comp, filt, inter) == (8, 6, 0, 0, 0)
            elif tag == b"IDAT":
                idat += body
            pos += 12 + n
        rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + 4 * W)
        assert (rows[:, 0] == 0).all()
        return rows[:, 1:].reshape(H, W, 4)
