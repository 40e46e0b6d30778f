"""Generates the forecast-rendering fixtures under tests/golden/ with the libraries the REFERENCE's pic_results.py uses (numpy,
matplotlib; PIL to read the PNG back), by running its OWN vis_res and gray2color (pic_results.py:93-184), which are taken out of its
syntax tree and compiled by themselves; their steps are:

    (seq * PIXEL_SCALE).astype(np.uint8)  ->  seq[1::2]  ->  ListedColormap / BoundaryNorm  ->  frames side by side with a gap of ones
    ->  plt.imsave to a PNG  ->  the decoded 8-bit RGBA bytes.

pic_results.py cannot be imported (it runs at import time and needs the dataset), so its two settings blocks (:44-57 LAPS, :59-89
Shanghai) are read from its syntax tree with ast.literal_eval and written out as DATA:

    forecast_palette_shanghai.json / forecast_palette_laps.json   {"bounds": [...], "rgba": [[r, g, b, a], ...]}
    forecast_render_shanghai.npz   / forecast_render_laps.npz     pred, fields, strip and the call's settings

Needs the reference tree (ADNM_REFERENCE_ROOT), matplotlib and PIL; runs on the CPU.  The output is byte-identical from run to run
(fixed seeds, fixed zip timestamps).  Run:  python tools/make_golden_forecast.py
"""
import ast
import io
import json
import os
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
REF_ROOT = os.environ.get("ADNM_REFERENCE_ROOT", "/root/reference")
GAP = 10


def settings():
    """-> {"LAPS": {...}, "Shanghai": {...}}: the literal assignments of the two `dataset == ...` branches of pic_results.py"""
    tree = ast.parse(open(os.path.join(REF_ROOT, "pic_results.py")).read())
    out = {}

    def literal(node):
        # np.array([...]) / 255 and colors.ListedColormap([...]): the list inside is the setting
        if isinstance(node, ast.BinOp):
            return literal(node.left)
        if isinstance(node, ast.Call):
            return literal(node.args[0])
        return ast.literal_eval(node)

    def walk_if(node):
        test = node.test
        if (isinstance(test, ast.Compare) and isinstance(test.left, ast.Name) and test.left.id == "dataset" and len(test.comparators) == 1
                and isinstance(test.comparators[0], ast.Constant)):
            name, vals = test.comparators[0].value, {}
            for stmt in node.body:
                if isinstance(stmt, ast.Assign) and len(stmt.targets) == 1 and isinstance(stmt.targets[0], ast.Name):
                    try:
                        vals[stmt.targets[0].id] = literal(stmt.value)
                    except (ValueError, IndexError):
                        pass
            out[name] = vals
            for nxt in node.orelse:
                if isinstance(nxt, ast.If):
                    walk_if(nxt)

    for node in tree.body:
        if isinstance(node, ast.If):
            walk_if(node)
    return out


def reference_functions(bounds, color_map):
    """pic_results.py's own vis_res and gray2color, taken out of its syntax tree and compiled on their own (the module cannot be
    imported) with the globals they read: nothing of them is restated here"""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import torch
    from matplotlib import colors
    tree = ast.parse(open(os.path.join(REF_ROOT, "pic_results.py")).read())
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("vis_res", "gray2color")]
    assert sorted(n.name for n in defs) == ["gray2color", "vis_res"]
    ns = {"np": np, "plt": plt, "colors": colors, "torch": torch, "os": os, "BOUNDS": bounds, "COLOR_MAP": color_map}
    exec(compile(ast.Module(body=defs, type_ignores=[]), "pic_results.py", "exec"), ns)
    return ns["vis_res"], ns["gray2color"]


def reference_png(seq, pixel_scale, even_index_only, cmap, bounds, color_map):
    """one sample (T, H, W) fp32 through the reference's vis_res -> the PNG it wrote, decoded: (H, Ws, 4) uint8"""
    import tempfile
    from PIL import Image
    vis_res, gray2color = reference_functions(bounds, color_map)
    with tempfile.TemporaryDirectory() as d:
        vis_res(seq, save_path=d, pic_name="pred", pixel_scale=pixel_scale, gray2color=gray2color, cmap=cmap, gap=GAP, even_index_only=even_index_only)
        img = Image.open(os.path.join(d, "pred.png"))
        assert img.mode == "RGBA", img.mode
        return np.asarray(img, dtype=np.uint8)


def reference_fields(pred, pixel_scale, bounds):
    """the byte per pixel a consumer keeps: the reference's own quantisation, or (float form) BoundaryNorm's bin"""
    from matplotlib import colors
    if pixel_scale is not None:
        return (pred * pixel_scale).astype(np.uint8)
    K = len(bounds) - 1
    return np.clip(np.ma.filled(colors.BoundaryNorm(bounds, K)(pred), 0), 0, K - 1).astype(np.uint8)


def f32_neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


def planted_shanghai(bounds, scale):
    vals = [np.float32(0.0), np.float32(1.0)]
    for e in bounds:
        vals += f32_neighbours(np.float32(e / scale))
    s = np.float32(scale)
    for m in range(1, int(scale)):
        x, below = np.float32(m / scale), np.nextafter(np.float32(m), np.float32(0))
        for _ in range(8):   # the largest float whose fp32 product with the scale is one ulp below the integer m
            if x * s <= below:
                break
            x = np.nextafter(x, np.float32(0))
        if x * s == below:
            vals.append(x)
    vals = [v for v in vals if 0.0 <= v and v * s < 256.0]   # the uint8 cast of anything else is undefined in numpy
    return np.array(vals, dtype=np.float32)


def planted_laps(bounds):
    vals = [np.float32(0.0), np.float32(1.0)]
    for e in bounds:
        vals += f32_neighbours(np.float32(e))
    return np.array(vals, dtype=np.float32)


def save_npz(name, **arrays):
    """np.savez_compressed with fixed timestamps: the file is the same bytes on every run"""
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def save_palette(name, bounds, rgba):
    path = os.path.join(OUT, f"forecast_palette_{name}.json")
    with open(path, "w") as f:
        f.write(json.dumps({"bounds": [float(b) for b in bounds], "rgba": np.asarray(rgba).tolist()}) + "\n")
    print(f"forecast_palette_{name}: {len(rgba)} colours")


def case(name, shape, seed, planted, rgba, bounds, cmap, color_map, pixel_scale, even_index_only):
    rng = np.random.default_rng(seed)
    pred = rng.random(shape, dtype=np.float32)
    hw = shape[2] * shape[3]
    assert planted.size <= hw, (planted.size, hw)
    for t in (0, 1):   # frame 1 is in the strip with and without the frame selection; frame 0 only in the fields when it is on
        pred[0, t].reshape(-1)[:planted.size] = planted
    pred[1, shape[1] - 1].reshape(-1)[hw - planted.size:] = planted[::-1]
    strip = np.stack([reference_png(pred[b], pixel_scale, even_index_only, cmap, bounds, color_map) for b in range(shape[0])])
    fields = reference_fields(pred, pixel_scale, bounds)
    # the table written to the JSON file is the table matplotlib put into the PNG: every pixel that is not gap is one of its rows
    start, step = (1, 2) if even_index_only else (0, 1)
    assert {tuple(c) for c in strip.reshape(-1, 4)} <= {tuple(c) for c in np.asarray(rgba, dtype=np.uint8)} | {(255, 255, 255, 255)}
    save_npz(f"forecast_render_{name}", pred=pred, fields=fields, strip=strip, pixel_scale=np.float32(pixel_scale or 0.0), frame_start=np.int64(start),
             frame_step=np.int64(step), gap=np.int64(GAP))


def main():
    from matplotlib import colors
    s = settings()
    sh, la = s["Shanghai"], s["LAPS"]
    rows = np.asarray(sh["COLOR_MAP"], dtype=np.uint8)
    assert np.array_equal((np.asarray(sh["COLOR_MAP"]) / 255 * 255).astype(np.uint8), rows)
    save_palette("shanghai", sh["BOUNDS"], rows)
    color_map = np.asarray(sh["COLOR_MAP"]) / 255            # as pic_results.py:66-83 forms it; its gray2color builds the colormap (cmap=None)
    case("shanghai", (2, 20, 16, 12), 20, planted_shanghai(sh["BOUNDS"], sh["PIXEL_SCALE"]), rows, sh["BOUNDS"], sh["cmap"], color_map,
         sh["PIXEL_SCALE"], sh["even_index_only"])
    names = la["cmap"]
    rows = (np.array([colors.to_rgba(n) for n in names]) * 255).astype(np.uint8)
    save_palette("laps", la["BOUNDS"], rows)
    case("laps", (2, 3, 16, 12), 3, planted_laps(la["BOUNDS"]), rows, la["BOUNDS"], colors.ListedColormap(names), None, la["PIXEL_SCALE"], la["even_index_only"])


if __name__ == "__main__":
    main()
