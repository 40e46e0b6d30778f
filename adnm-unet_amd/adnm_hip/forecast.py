"""The output side of the hot path: the reference's third script, pic_results.py, loads the best checkpoint, forecasts the test set,
copies every prediction to numpy as floats and colours it frame by frame with matplotlib (vis_res, pic_results.py:104-184).  Here

    pal = Palette(BOUNDS, COLOR_MAP)                              # the caller's own table: the package ships none
    fc = Forecaster(model, pal, pixel_scale=90.0, size=128, frame_start=1, frame_step=2)
    res = fc(x)                 # ONE replay of a captured graph; x: fp32 (B, T_in, 1, S, S) or RAW uint8 (B, T_in, H0, W0) on the device
    res.pred, res.fields, res.strip                               # fp32 forecast, a byte per pixel, the RGBA colour strip
    fc.save(out_dir, res, "ADNMUnet", batch=cnt)                  # {batch}-{i+1}/ADNMUnet.png, as pic_results.py:263-271 lays them out
    fc.save(out_dir, fc.render(targets), "gt", batch=cnt)         # the gt.png row: the same palette on any other (B, T, ...) tensor

A call is GraphedForward's captured graph with csrc/dataio.hip::forecast_render behind the forward (ForwardClient.after; one launch: the
quantised fields, the frame selection, the colour lookup, the gaps) and, for raw bytes, adnm_radar_ingest in front of it (model_input).
What leaves the device is 1 + 4 n / T bytes per pixel (n of T frames selected) instead of 4, and the host does no per-frame work.

The value rule is stated in include/adnm_hip.h (adnm_forecast_render); inside the uint8 range it is pic_results.py's, byte for byte
(tests/golden/forecast_render_*.npz are matplotlib's own output).  Figure layout beyond the strip and LPIPS are not reproduced."""
import ctypes
import json
import os
import struct
import zlib

import numpy as np
import torch

from . import lib, ops
from .evaluator import ForwardClient, GraphedForward

MAX_BINS = 32


class Palette:
    """BoundaryNorm(bounds, K) + ListedColormap(colours) as a table: K + 1 ascending edges, K RGBA rows.  colours: (K, 4) uint8, or
    floats in [0, 1] converted with (c * 255).astype(uint8) as matplotlib does.  `edges` keeps the doubles as given; `bounds` is what
    the kernel compares against: each edge rounded UP to the smallest float32 >= it (ops.edges_up_f32)."""

    def __init__(self, bounds, colours):
        self.edges = tuple(float(e) for e in bounds)
        c = np.asarray(colours)
        if c.ndim != 2 or c.shape[1] != 4:
            raise ValueError(f"Palette: colours must be (K, 4) RGBA rows, got {c.shape}")
        if c.dtype.kind == "f":
            if not (np.isfinite(c).all() and c.min() >= 0.0 and c.max() <= 1.0):
                raise ValueError("Palette: float colours must lie in [0, 1]")
            c = (c * 255).astype(np.uint8)
        elif c.dtype.kind in "iu":
            if c.min() < 0 or c.max() > 255:
                raise ValueError("Palette: integer colours must lie in 0..255")
            c = c.astype(np.uint8)
        else:
            raise ValueError(f"Palette: colours must be uint8 or floats in [0, 1], got {c.dtype}")
        K = c.shape[0]
        if not 1 <= K <= MAX_BINS:
            raise ValueError(f"Palette: 1..{MAX_BINS} colours, got {K}")
        if len(self.edges) != K + 1:
            raise ValueError(f"Palette: {K} colours need {K + 1} edges, got {len(self.edges)}")
        self.colours = np.ascontiguousarray(c)
        self.bounds = ops.edges_up_f32(self.edges)
        if not (np.diff(self.bounds) > 0).all():
            raise ValueError("Palette: the edges must be strictly ascending (as float32 too)")
        self._c = ops.render_tables(self.edges, self.colours)   # the host tables as the entry point reads them, made once

    @property
    def nbins(self):
        return self.colours.shape[0]

    # the JSON form of tests/golden/forecast_palette_*.json: the edges and the 8-bit RGBA rows, nothing else
    def to_json(self):
        return json.dumps({"bounds": list(self.edges), "rgba": self.colours.tolist()})

    @classmethod
    def from_json(cls, text):
        d = json.loads(text)
        if set(d) != {"bounds", "rgba"}:
            raise ValueError(f"Palette: expected the keys 'bounds' and 'rgba', got {sorted(d)}")
        return cls(d["bounds"], np.asarray(d["rgba"], dtype=np.int64))

    def save(self, path):
        with open(path, "w") as f:
            f.write(self.to_json() + "\n")

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls.from_json(f.read())

    def __eq__(self, other):
        return isinstance(other, Palette) and self.edges == other.edges and np.array_equal(self.colours, other.colours)


def save_png(path, rgba_u8):
    """An (H, W, 4) uint8 array (numpy or a tensor on any device) -> an 8-bit RGBA PNG, with the standard library only (what plt.imsave
    writes for pic_results.py, without matplotlib on the machine that forecasts)."""
    a = rgba_u8.detach().cpu().numpy() if torch.is_tensor(rgba_u8) else np.asarray(rgba_u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"save_png: needs a uint8 (H, W, 4) image, got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + 4 * W), dtype=np.uint8)          # filter type 0 in front of every scanline
    rows[:, 1:] = a.reshape(H, 4 * W)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6))
           + chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)


class Forecast:
    """What a Forecaster call returns: .pred (fp32, the model's output in the model's own shape: (B, T, 1, H, W) from create_ADNMUNet's
    models, (B, T, H, W) from a model that emits that; for render() the tensor it was given), .fields (uint8 (B, T, H, W)),
    .strip (uint8 (B, H, Ws, 4)), and .prob (fp32 (K, B, T, H, W), the neighbourhood probability per threshold of a Forecaster with
    probability=; None otherwise).  With ensemble=: .members (fp32 (M, B, T, H, W), the member forecasts with their symmetries undone, member 0
    the control), .ens_mean (fp32 (B, T, H, W)) and .ens_prob (fp32 (K, B, T, H, W), the share of members at or above each threshold; None
    without thresholds); .pred, .fields, .strip and .prob are then the control's.  None otherwise."""
    __slots__ = ("pred", "fields", "strip", "prob", "members", "ens_mean", "ens_prob")

    def __init__(self, pred, fields, strip, prob=None, members=None, ens_mean=None, ens_prob=None):
        self.pred, self.fields, self.strip, self.prob = pred, fields, strip, prob
        self.members, self.ens_mean, self.ens_prob = members, ens_mean, ens_prob


class Forecaster(ForwardClient):
    def __init__(self, model, palette, pixel_scale=90.0, size=None, in_frames=5, frame_start=0, frame_step=1, gap=10, probability=None, ensemble=None):
        """pixel_scale: pic_results.py's PIXEL_SCALE; None or 0 bins the float itself (the LAPS form).  size: the model's input edge,
        needed for raw uint8 input only.  frame_start / frame_step: the frames of the strip (even_index_only=True is 1, 2).
        probability: dict(thresholds=(35, 40), scale=9) adds Forecast.prob, the fraction of the scale x scale window at or above each
        threshold on the field quantised with pixel_scale: one adnm_neighbour_prob launch behind the render, in the graph.
        ensemble: dict(members=True | codes, thresholds=(35, 40)) forecasts a test-time-augmentation ensemble over the symmetries of the square
        (the member recipe is the Validator's, ops.ensemble_spec): the forward runs at batch M * B on the transformed inputs,
        adnm_d4_members undoes the symmetries, and one adnm_ensemble_product launch behind the render writes Forecast.ens_mean and, with
        thresholds (on the field quantised with pixel_scale), Forecast.ens_prob.  render(res.ens_mean) colours the mean."""
        if not isinstance(palette, Palette):
            raise RuntimeError(f"Forecaster: palette must be a forecast.Palette, got {type(palette).__name__}")
        self.model, self.palette = model, palette
        self.pixel_scale = 0.0 if pixel_scale is None else float(pixel_scale)
        self.size, self.in_frames = (None if size is None else int(size)), int(in_frames)
        self.frame_start, self.frame_step, self.gap = int(frame_start), int(frame_step), int(gap)
        if not (self.pixel_scale >= 0.0 and np.isfinite(self.pixel_scale)) or self.frame_start < 0 or self.frame_step < 1 or self.gap < 0:
            raise ValueError("Forecaster: pixel_scale >= 0, frame_start >= 0, frame_step >= 1, gap >= 0")
        self.probability = None             # (thresholds as the entry point reads them, K, scale)
        if probability is not None:
            if not isinstance(probability, dict) or set(probability) != {"thresholds", "scale"}:
                raise ValueError(f"Forecaster: probability is dict(thresholds=, scale=), got {probability!r}")
            if not self.pixel_scale > 0.0:
                raise ValueError("Forecaster: probability= compares the field quantised with pixel_scale, which must be > 0 (not None or 0)")
            thr, scales = [float(t) for t in probability["thresholds"]], ops.fss_scales(probability["scale"])
            if len(scales) != 1 or not 1 <= len(thr) <= 8:
                raise ValueError("Forecaster: probability takes one scale and 1..8 thresholds")
            self.probability = ((ctypes.c_float * len(thr))(*thr), len(thr), scales[0])
        self.ensemble = None                # (the members argument, thresholds as the entry point reads them, K)
        if ensemble is not None:
            if not isinstance(ensemble, dict) or "members" not in ensemble or not set(ensemble) <= {"members", "thresholds"}:
                raise ValueError(f"Forecaster: ensemble is dict(members=, thresholds=), got {ensemble!r}")
            members = ops.ensemble_spec(ensemble["members"], None)   # ValueError on a bad entry
            thr = [float(t) for t in ensemble.get("thresholds") or ()]
            if members is None or len(thr) > 8:
                raise ValueError("Forecaster: ensemble takes members (True or codes) and 0..8 thresholds")
            if thr and not self.pixel_scale > 0.0:
                raise ValueError("Forecaster: the ensemble's thresholds compare the field quantised with pixel_scale, which must be > 0 (not None or 0)")
            self.ensemble = (members, (ctypes.c_float * max(len(thr), 1))(*thr), len(thr))
        self.out_frames = None              # T of the model's output, known after the first call
        self._fwd = GraphedForward(model, client=self, keep_quant=True)
        self._warm = set()                  # the devices the render kernel has run on

    # ---- ForwardClient: what GraphedForward calls with the entry of one input shape
    def open(self, ent, x):
        """both variants of the render kernel run once before a capture launches them (a kernel's first launch must not be captured);
        raw bytes: the fp32 tensor adnm_radar_ingest fills for the model"""
        if x.device not in self._warm:
            for w in (4, 1):
                ops.forecast_render_tables(torch.zeros((1, 1, 1, w), dtype=torch.float32, device=x.device), self.palette._c, self.pixel_scale, gap=0)
                if self.probability:   # likewise the probability kernel, aligned and not
                    ops.neighbour_prob_into(torch.zeros((1, 1, 1, w), dtype=torch.float32, device=x.device),
                                            torch.empty((self.probability[1], 1, 1, 1, w), dtype=torch.float32, device=x.device), *self.probability[:2],
                                            self.pixel_scale, self.probability[2])
            self._warm.add(x.device)
        raw = x.dtype == torch.uint8
        ent["xin"] = torch.empty((x.shape[0], x.shape[1], 1, self.size, self.size), dtype=torch.float32, device=x.device) if raw else None
        ent["codes"] = ent["xmem"] = None
        if self.ensemble:   # the members' inputs, made from the ingested frames; the forward direction once, eagerly
            first = ent["xin"] if raw else ent["sx"]
            H, W = first.shape[-2:]
            codes = ops.ensemble_spec(self.ensemble[0], H == W)   # ValueError: a transposing code on frames that are not square
            if first.numel() // (H * W) > 65535:
                raise RuntimeError(f"Forecaster: ensemble= on {first.numel() // (H * W)} input frames is outside adnm_d4_members' limits (<= 65535)")
            ent["codes"] = (ctypes.c_int * len(codes))(*codes)
            ent["xmem"] = torch.zeros((len(codes) * first.shape[0],) + tuple(first.shape[1:]), dtype=torch.float32, device=x.device)
            ops.d4_members_into(first, ent["xmem"], ent["codes"], len(codes), False)

    def model_input(self, ent, sx):
        """raw bytes: ingest first; ensemble: then the M transformed copies, member-major (sample m * B + b is member m of sample b)"""
        first = sx
        if ent["xin"] is not None:
            B, T, H0, W0 = sx.shape
            lib.call("adnm_radar_ingest", sx.data_ptr(), ent["xin"].data_ptr(), B * T, H0, W0, self.size, 1.0 / 255.0, torch.cuda.current_stream().cuda_stream)
            first = ent["xin"]
        if ent["xmem"] is None:
            return first
        ops.d4_members_into(first, ent["xmem"], ent["codes"], len(ent["codes"]), False)
        return ent["xmem"]

    def check(self, ent, out):
        """the checks that may raise, and the buffers after() writes"""
        if out.dtype != torch.float32 or out.dim() not in (4, 5) or (out.dim() == 5 and out.shape[2] != 1):
            raise RuntimeError(f"Forecaster: the model's output must be fp32 (B, T, H, W) or (B, T, 1, H, W), got {out.dtype} {tuple(out.shape)}")
        B, T, H, W = out.shape[0], out.shape[1], out.shape[-2], out.shape[-1]
        ent["members"] = ent["ens_mean"] = ent["ens_prob"] = None
        if ent["codes"] is not None:   # the members' buffers, and the inverse direction and the product once, eagerly
            M, K = len(ent["codes"]), self.ensemble[2]
            if B % M or (H != W and any(c & 4 for c in ent["codes"])) or B * T > 65535 * M or H * W >= 1 << 24:
                raise RuntimeError(f"Forecaster: ensemble= of {M} members does not fit the model's output {tuple(out.shape)} (batch M * B, square frames for a "
                                   "transposing member, B * T <= 65535, H * W < 2^24)")
            B //= M
            ent["members"] = torch.zeros((M, B, T, H, W), dtype=torch.float32, device=out.device)
            ent["ens_mean"] = torch.empty((B, T, H, W), dtype=torch.float32, device=out.device)
            ent["ens_prob"] = torch.empty((K, B, T, H, W), dtype=torch.float32, device=out.device) if K else None
            ops.d4_members_into(torch.zeros_like(ent["members"]), ent["members"], ent["codes"], M, True)
            self._product(ent)
        if self.frame_start >= T:
            raise RuntimeError(f"Forecaster: frame_start {self.frame_start} outside the model's {T} output frames")
        ent["fields"] = torch.empty((B, T, H, W), dtype=torch.uint8, device=out.device)
        ent["strip"] = torch.empty((B, H, ops.strip_width(T, W, self.frame_start, self.frame_step, self.gap), 4), dtype=torch.uint8, device=out.device)
        ent["prob"] = torch.empty((self.probability[1], B, T, H, W), dtype=torch.float32, device=out.device) if self.probability else None

    def _product(self, ent):
        M, B, T, H, W = ent["members"].shape
        ops.ensemble_product_into(ent["members"], B * T * H * W, T * H * W, H * W, ent["ens_mean"], ent["ens_prob"], self.ensemble[1], self.ensemble[2],
                                  self.pixel_scale, M, B * T, T, H * W)

    def after(self, ent, sx, out):
        ent["keep"] = pred = (out.squeeze(2) if out.dim() == 5 else out).contiguous()   # (a copy made here belongs to the graph's pool and is kept with it)
        if ent["members"] is not None:   # the symmetries undone; what follows renders member 0, the contiguous control forecast
            mem = ent["members"]
            ops.d4_members_into(pred, mem, ent["codes"], mem.shape[0], True)
            pred = mem[0]
            out = pred.view((mem.shape[1],) + tuple(out.shape[1:]))   # in the model's own shape
        ops.forecast_render_into(pred, ent["fields"], ent["strip"], self.palette._c, self.pixel_scale, self.frame_start, self.frame_step, self.gap)
        if self.probability:
            ops.neighbour_prob_into(pred, ent["prob"], *self.probability[:2], self.pixel_scale, self.probability[2])
        if ent["members"] is not None:
            self._product(ent)
        ent["res"] = Forecast(out, ent["fields"], ent["strip"], ent["prob"], ent["members"], ent["ens_mean"], ent["ens_prob"])
        self.out_frames = out.shape[1]

    # ---- the public surface
    @torch.no_grad()
    def __call__(self, x):
        """x: fp32 (B, in_frames, 1, S, S), or raw uint8 (B, in_frames, H0, W0) radar frames (then / 255 and the bilinear resize to
        `size` run inside the same graph), on the GPU.  -> Forecast(pred, fields, strip, prob): STATIC buffers of the graph of this input
        shape, valid until the next call with that shape (copy what has to last)."""
        if not (torch.is_tensor(x) and x.is_cuda):
            raise RuntimeError("Forecaster runs on GPU tensors only (there is no CPU path here)")
        if x.dtype == torch.uint8:
            if x.dim() != 4:
                raise RuntimeError(f"Forecaster: raw input must be uint8 (B, T_in, H0, W0), got {tuple(x.shape)}")
            if self.size is None:
                raise RuntimeError("Forecaster: raw uint8 input needs size= (the model's input edge)")
        elif x.dtype != torch.float32 or x.dim() != 5 or x.shape[2] != 1:
            raise RuntimeError(f"Forecaster: input must be fp32 (B, T_in, 1, S, S) or raw uint8 (B, T_in, H0, W0), got {x.dtype} {tuple(x.shape)}")
        if x.shape[1] != self.in_frames:
            raise RuntimeError(f"Forecaster: the input has {x.shape[1]} frames per sample, in_frames is {self.in_frames}")
        x = x.contiguous()
        return self._fwd.replay(self._fwd.entry(x), x)["res"]

    def render(self, t, frame_start=None, frame_step=None):
        """The same palette, pixel_scale and gap on any other (B, T, H, W) / (B, T, 1, H, W) fp32 GPU tensor -> a Forecast whose .pred is
        `t` (freshly allocated outputs, one launch).  With the Forecaster's own frame selection (the default) `t` must have the
        forecast's T — the gt.png row; give frame_start=0, frame_step=1 for the input.png row, which keeps every frame."""
        own = frame_start is None and frame_step is None
        fs = self.frame_start if frame_start is None else int(frame_start)
        step = self.frame_step if frame_step is None else int(frame_step)
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError("Forecaster runs on GPU tensors only (there is no CPU path here)")
        if own and self.out_frames is not None and t.dim() >= 2 and t.shape[1] != self.out_frames:
            raise RuntimeError(f"Forecaster.render: {t.shape[1]} frames per sample, but the frame selection was built for the forecast's {self.out_frames} "
                               "(pass frame_start / frame_step for another sequence)")
        fields, strip = ops.forecast_render_tables(t, self.palette._c, self.pixel_scale, fs, step, self.gap)
        return Forecast(t, fields, strip)

    def save(self, directory, result, name, batch=1):
        """result.strip -> {directory}/{batch}-{i+1}/{name}.png per sample i (pic_results.py:263-271).  One device -> host copy."""
        strips = result.strip.cpu().numpy()
        paths = []
        for i in range(strips.shape[0]):
            d = os.path.join(directory, f"{batch}-{i + 1}")
            os.makedirs(d, exist_ok=True)
            paths.append(os.path.join(d, f"{name}.png"))
            save_png(paths[-1], strips[i])
        return paths

    def close(self):
        """Give the captured graphs and their static buffers back (GraphedForward.close).  Idempotent; __del__ calls it."""
        self._fwd.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
