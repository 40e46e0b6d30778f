"""The validation half of an epoch on the device (train.py:156-206 of the reference: a forward-only pass over the validation set, the
loss per batch, the metrics, then the best-checkpoint rule and the early stop).

    val = Validator(model, loss_fn, seq_len, value_scale, thresholds=(20, 30, 35, 40), ssim=True, process_group=None)
    for x, tgt in val_loader:
        val.step(x, tgt)          # one replay of a captured graph: no allocation, no host synchronisation
    res = val.done(reset=True)    # the one synchronising read of the epoch
    decision = selection.update(epoch, res["loss_sum"])      # ReferenceSelection (adnm_hip.schedule)

A step is GraphedForward's captured graph with a second body behind the forward (ForwardClient.after): csrc/dataio.hip::valid_accum (the enRainfallLoss
value of the batch — no gradient tensor — and SimplifiedEvaluator's contingency counts and error sums, one pass over prediction and
target) and valid_ssim_accum, both ADDING into one block of doubles that lives on the device for the epoch (layout:
include/adnm_hip.h, adnm_valid_accum).  done() reads that block — summed over the ranks of `process_group` with one all-reduce —
and aggregates it exactly as GpuEvaluator.done() does.

Every option below adds tables of its own behind that block, in the same allocation.  block_parts is the ONE statement of which tables
there are and where each lies: the allocation, the launches (one per table, in the table's order) and aggregate all read it (through
block_rows, which states the rows; block_tables, block_layout and block_parts keep the parameter lists they had before later tables arrived).  The defaults
allocate and launch nothing new.

Validator(..., pools=(4, 16, (16, 8)), persistence=True) adds neighbourhood scores and the persistence baseline:
csrc/dataio.hip::valid_pool_accum counts TP / FN / FP / TN per window of a spatial max-pool, for the forecast and for the last input
frame held over the horizon; done(per_lead=True) adds every score per frame index, from the rows the block always kept.

Validator(..., fss=(1, 5, 17, 33)) adds the Fractions Skill Score per scale and threshold: csrc/dataio.hip::valid_fss_accum
adds the integer sums A = sum c_o^2, F = sum c_f^2, C = sum c_o c_f of the windowed event counts (for the forecast, and with persistence
for the baseline), and done() reports FSS = 2C / (A + F) from the summed rows.

Validator(..., advection=True) adds the Lagrangian-persistence baseline: csrc/advect.hip::trec_cost / trec_pick estimate one
motion vector per block from the last two input frames, advect moves the last frame along it for every frame index, and that field is
scored as a second baseline by the same pooled and FSS passes.  With advection_flow=True the field comes from
csrc/flow.hip instead: trec_flow refines each vector to 1/16 px on the same cost tables and advect_flow carries the last frame backwards
along the dense field between the block centres, one step per frame, with four taps in fp32; tables, passes and keys stay where they were.

Validator(..., spectrum=True) adds radially averaged power spectra: csrc/spectrum.hip::valid_spectrum_accum transforms the
clipped, scaled target and forecast (power-of-two frames of 8..512 pixels a side) and adds the power of each and their co-spectrum per
radial wavenumber and frame index; done() reports the mean power per coefficient, the forecast's share of the observed power, the
spectral coherence and the scale down to which the forecast keeps half the observed power.

Validator(..., joint=True) adds the joint intensity histogram: csrc/joint.hip::valid_joint_accum counts, per frame index, the
pixels at every pair (quantised target, quantised forecast) into a (T, L, L) table, L = floor(value_scale) + 1; done() derives the
contingency table and the scores at EVERY integer threshold, the frequency bias, the conditional mean, a quantile-mapping table and the
correlation from it (joint_entries), and joint_counts_at gives the counts at any threshold.

Validator(..., objects=True) (or objects=min_area) adds object-based scores: csrc/objects.hip::valid_objects_accum labels the
8-connected components of the event mask of every frame, threshold and field (target, forecast) on the device and adds, per frame index, the
number of objects, their areas, squared areas, the largest one, the objects the other field touches and a size histogram into a
(T, 2, nthr, 23) table; done() reports counts, mean and area-weighted sizes, count and size bias and the object POD / FAR / CSI
(object_entries).

Validator(..., sal=True) (or sal=min_area, or sal=dict(min_area=, intensity=)) adds the SAL scores: csrc/sal.hip::valid_sal_accum
labels the same objects, gives each the sum, the maximum and the first moments of an intensity weight, forms Structure, Amplitude and Location
per frame pair and threshold and adds them, with the number of frames each is defined on, into a (T, nthr, 12) table; done() reports the
means (sal_entries).

Validator(..., nprob=(1, 5, 17, 33)) (or nprob=True for the fss scales) adds the neighbourhood exceedance probability's verification
(DESIGN.md §4r): csrc/neighbour.hip::valid_nprob_accum counts, per frame index, threshold and scale, the pixels by (observed event bit,
forecast events in the n x n window) into a (T, nthr, S) table of integers; done() reports the Brier score and its decomposition, the ROC
curve and its area and the reliability diagram of p = count / n^2 (nprob_entries).

Validator(..., tracks=True) (or tracks=min_volume, or tracks=dict(min_volume=)) adds space-time rain-cell tracks:
csrc/tracks.hip::valid_tracks_accum labels the 26-connected components of every sample's (T, H, W) event volume, per threshold and field, on the
device and adds the number of tracks, their volumes and durations, the matched ones, births and deaths per frame index, the deaths of the tracks
present at the first lead and a duration histogram into a (2, nthr, 7 + 4 T) table; done() reports lifetimes, the survival curve of the initial
cells and the track POD / FAR / CSI (track_entries).

Validator(..., intensity_scale=True) adds the intensity-scale skill score: csrc/neighbour.hip::valid_iscale_accum adds, per frame
index, threshold and level l = 0 .. L, the integer sums A, F, C of the squared event counts over the 2^l x 2^l blocks of the zero-padded
P x P domain into a (T, L + 1, 3 nthr) table, for the forecast and for each baseline there is; done() reports the MSE, the skill and the
energies of the binary error's Haar components of scale 1, 2, 4, ... P px (intensity_scale_entries).

Validator(..., ensemble=True) (or ensemble=codes, or ensemble=dict(members=codes)) scores a test-time-augmentation ensemble over the symmetries
of the square: csrc/ensemble.hip::d4_members puts the M transformed copies of the input in front of the forward, which then runs at
batch M * B, and undoes the symmetries on its output; valid_ens_accum adds the integer sums behind CRPS, spread and skill, the rank histogram and
the ensemble exceedance probability's histogram into a (T, C) table; done() reports them (ensemble_entries).  Every other pass scores member 0,
the control: the model on the untouched input, though at batch M * B, where the GEMM plans may differ from those at batch B, so it is NOT
promised bit-equal to a plain Validator's forecast.

The reference's loop iterates `for batch in val_dataloader` but evaluates `data`, the last TRAINING batch (train.py:159-160).  That is
not reproduced: the Validator validates the batches it is given."""
import ctypes
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import lib, ops
from .evaluator import ForwardClient, GraphedForward, contingency_metrics

HEADER = 4   # doubles in front of the table: loss_sum, batches, samples, nonfinite_batches


def reduce_block(block, process_group=None):
    """The multi-rank step of Validator.done(): `block` (a float64 tensor on any device, gloo on the CPU included) becomes the
    elementwise sum over the ranks of `process_group`, in place, with ONE all-reduce; every rank then holds the same block.  Counts are
    integers in doubles and the loss sums are sums of fp32 values: the result does not depend on the ranks' order beyond the last bit
    of the float columns.  process_group None: nothing to do."""
    if process_group is not None:
        import torch.distributed as dist
        if block.dtype != torch.float64:
            raise RuntimeError(f"reduce_block: the accumulator block is float64, got {block.dtype}")
        dist.all_reduce(block, op=dist.ReduceOp.SUM, group=process_group)
    return block


def baseline_pools(pools):
    """the pools the persistence baseline is scored at: point-wise first, then every pool of the forecast"""
    return ((1, 1),) + tuple(p for p in pools if p != (1, 1))


class Part(NamedTuple):
    """one table of the Validator's block: `kind` is main / pool / fss / spectrum / joint / objects / sal / nprob / iscale / ensemble / tracks, `field` the field it scores against the target
    (pred: the forecast, last: the last input frame held, adv: that frame advected; None for main), `pools` the (size, stride) pairs of a
    pool part's pass, `offset` its place in the block in doubles"""
    name: str
    kind: str
    field: Optional[str]
    pools: tuple
    shape: tuple
    offset: int

    @property
    def size(self):
        return math.prod(self.shape)


def block_rows(T, nthr, pools=(), persistence=False, fss=(), advection=False, spectrum=None, joint=None, sal=None, nprob=None, tracks=None, objects=None,
               iscale=None, ensemble=None):
    """-> (the parts of the ONE allocation in their order, its doubles).  The order of the block, and of the launches that fill it, is stated
    here and nowhere else: block_tables, block_layout and block_parts are its callers with the parameter lists they had, the Validator and
    aggregate go through this one.  ensemble: the number of members M, or None; BY NAME: the ensemble's table (T, C), C from
    ops.ensemble_cols(M, nthr), directly in front of the tracks.  pools: (size, stride) pairs; fss: scales; spectrum: (H, W) of the frames, or None; joint: the levels L, or None;
    objects: min_area, or None; sal: what ops.sal_spec returns, or None.  `sal` is passed BY NAME: it stands in front of `objects`, which
    stays the last parameter, and its position may move when a further table arrives.  nprob: the scales of the neighbourhood probability's
    histogram, or None; passed BY NAME as well, for the same reason.  tracks: min_volume, or None; BY NAME too: its table, (2, nthr, 7 + 4 T)
    with no leading T axis, is the last one whatever its place here.  iscale: (H, W) of the frames, or None; BY NAME: the intensity-scale
    tables (T, L + 1, 3 * nthr), L from ops.intensity_scale_levels (ValueError outside its limits), of the forecast and of each baseline
    there is, directly in front of the tracks."""
    pools, fss, nprob = tuple(pools), tuple(fss), tuple(nprob or ())
    levels = (T, ops.intensity_scale_levels(*iscale)[1] + 1, 3 * nthr) if iscale else ()
    base = baseline_pools(pools)
    pooled, scaled = (T, len(base), 4 * nthr), (T, len(fss), 3 * nthr)
    rows = (("main", "main", None, (), (HEADER + T * (4 * nthr + 3),), True),
            ("pooled", "pool", "pred", pools, (T, len(pools), 4 * nthr), pools),
            ("persistence/pooled", "pool", "last", base, pooled, persistence),
            ("fss", "fss", "pred", (), scaled, fss),
            ("persistence/fss", "fss", "last", (), scaled, fss and persistence),
            ("advection/pooled", "pool", "adv", base, pooled, advection),
            ("advection/fss", "fss", "adv", (), scaled, fss and advection),
            ("spectrum", "spectrum", "pred", (), (T, max(spectrum) // 2, 3) if spectrum else (), spectrum),
            ("joint", "joint", "pred", (), (T, joint, joint), joint),
            ("objects", "objects", "pred", (), (T, 2, nthr, ops.OBJ_COLS), objects),
            ("sal", "sal", "pred", (), (T, nthr, ops.SAL_COLS), sal),
            ("nprob", "nprob", "pred", (), (T, nthr, ops.nprob_layout(nprob)[1]), nprob),
            ("iscale", "iscale", "pred", (), levels, iscale),
            ("persistence/iscale", "iscale", "last", (), levels, iscale and persistence),
            ("advection/iscale", "iscale", "adv", (), levels, iscale and advection),
            ("ensemble", "ensemble", "pred", (), (T, ops.ensemble_cols(ensemble, nthr)[0]) if ensemble else (), ensemble),
            ("tracks", "tracks", "pred", (), (2, nthr, ops.track_cols(T)[0]), tracks))
    parts, at = [], 0
    for *head, shape, present in rows:
        if present:
            parts.append(Part(*head, shape, at))
            at += parts[-1].size
    return parts, at


def block_tables(T, nthr, pools=(), persistence=False, fss=(), advection=False, spectrum=None, joint=None, sal=None, nprob=None, tracks=None, objects=None,
                 iscale=None):
    """block_rows without the table that came after the intensity-scale ones: the parameter list callers and tests have pinned."""
    return block_rows(T, nthr, pools, persistence, fss, advection, spectrum, joint, sal=sal, nprob=nprob, tracks=tracks, objects=objects, iscale=iscale)


def block_layout(T, nthr, pools=(), persistence=False, fss=(), advection=False, spectrum=None, joint=None, sal=None, nprob=None, tracks=None, objects=None):
    """block_tables without the tables that came after the tracks': the parameter list callers and tests have pinned."""
    return block_tables(T, nthr, pools, persistence, fss, advection, spectrum, joint, sal=sal, nprob=nprob, tracks=tracks, objects=objects)


def block_parts(T, nthr, pools=(), persistence=False, fss=(), advection=False, spectrum=None, joint=None, sal=None, nprob=None, objects=None):
    """block_tables without the tables that came after the neighbourhood probability's: the parameter list callers and tests have pinned.
    The Validator and aggregate go through block_rows, which states the rows."""
    return block_tables(T, nthr, pools, persistence, fss, advection, spectrum, joint, sal=sal, nprob=nprob, objects=objects)


def _doubles(names, *options, **more):
    """the doubles of the named parts of block_rows(*options, **more), 0 for a part that is not there"""
    size = {p.name: p.size for p in block_rows(*options, **more)[0]}
    return tuple(size.get(n, 0) for n in names)


def block_doubles(seq_len, nthr, pools=(), persistence=False):
    """-> (doubles of the main block, of the forecast's pooled table, of the baseline's)"""
    return _doubles(("main", "pooled", "persistence/pooled"), seq_len, nthr, pools, persistence)


def fss_doubles(seq_len, nthr, fss=(), persistence=False):
    """-> (doubles of the forecast's FSS table, of the baseline's)"""
    return _doubles(("fss", "persistence/fss"), seq_len, nthr, (), persistence, fss)


def advection_doubles(seq_len, nthr, pools=(), fss=(), advection=False):
    """-> (doubles of the advection baseline's pooled table, of its FSS table)"""
    return _doubles(("advection/pooled", "advection/fss"), seq_len, nthr, pools, fss=fss, advection=advection)


def spectrum_doubles(seq_len, frame=None):
    """-> doubles of the spectrum table (T, max(H, W) / 2, 3); frame: (H, W), or None / False for none"""
    return _doubles(("spectrum",), seq_len, 1, spectrum=frame)[0]


def joint_doubles(seq_len, value_scale=None):
    """-> doubles of the joint histogram (T, L, L), L = ops.joint_levels(value_scale); value_scale None / False for none"""
    none = value_scale is None or value_scale is False
    return _doubles(("joint",), seq_len, 1, joint=None if none else ops.joint_levels(value_scale))[0]


def objects_doubles(seq_len, nthr, objects=None):
    """-> doubles of the objects table (T, 2, nthr, ops.OBJ_COLS); objects: what ops.objects_spec takes (None / False for none)"""
    return _doubles(("objects",), seq_len, nthr, objects=ops.objects_spec(objects))[0]


def sal_doubles(seq_len, nthr, sal=None):
    """-> doubles of the SAL table (T, nthr, ops.SAL_COLS); sal: what ops.sal_spec takes (None / False for none)"""
    return _doubles(("sal",), seq_len, nthr, sal=ops.sal_spec(sal))[0]


def nprob_doubles(seq_len, nthr, nprob=None):
    """-> doubles of the neighbourhood probability's table (T, nthr, S), S = ops.nprob_layout(scales)[1]; nprob: the scales (None / () for none)"""
    return _doubles(("nprob",), seq_len, nthr, nprob=ops.fss_scales(nprob))[0]


def tracks_doubles(seq_len, nthr, tracks=None):
    """-> doubles of the tracks table (2, nthr, 7 + 4 T); tracks: what ops.tracks_spec takes (None / False for none)"""
    return _doubles(("tracks",), seq_len, nthr, tracks=ops.tracks_spec(tracks))[0]


def ensemble_doubles(seq_len, nthr, members=None):
    """-> doubles of the ensemble's table (T, C), C = ops.ensemble_cols(M, nthr)[0]; members: M (None / 0 for none)"""
    return _doubles(("ensemble",), seq_len, nthr, ensemble=members or None)[0]


def iscale_doubles(seq_len, nthr, frame=None, persistence=False, advection=False):
    """-> (doubles of the forecast's intensity-scale table (T, L + 1, 3 * nthr), of the persistence baseline's, of the advection baseline's);
    frame: (H, W), or None / False for none"""
    return _doubles(("iscale", "persistence/iscale", "advection/iscale"), seq_len, nthr, persistence=persistence, advection=advection, iscale=frame or None)


def _counts(hist):
    """a histogram as numpy int64 (..., L, L): a torch tensor (ops.joint_histogram's, on any device) or anything numpy takes; doubles holding
    integers (the Validator's table) are converted exactly"""
    if torch.is_tensor(hist):
        hist = hist.detach().cpu().numpy()
    h = np.asarray(hist)
    if h.ndim < 2 or h.shape[-1] != h.shape[-2] or h.shape[-1] < 1:
        raise ValueError(f"joint: a histogram is (..., L, L), got {h.shape}")
    if h.dtype.kind == "f":
        if not (np.isfinite(h).all() and (h == np.rint(h)).all()):
            raise ValueError("joint: a histogram holds integer counts")
    elif h.dtype.kind not in "iu":
        raise ValueError(f"joint: a histogram holds integer counts, got {h.dtype}")
    h = h.astype(np.int64)
    if (h < 0).any():
        raise ValueError("joint: a histogram holds counts >= 0")
    return h


def _tail_sums(a, axis):
    """s[v] = sum of a[u] over u >= v along `axis`"""
    return np.flip(np.cumsum(np.flip(a, axis), axis=axis), axis)


def _scalar(a):
    return a.item() if a.ndim == 0 else a


def joint_counts_at(hist, thr):
    """hist: (..., L, L) counts [q_o][q_f] (ops.joint_histogram's tensor, done()["joint"]["histogram"], ...) -> (TP, FN, FP, TN) at the float
    threshold thr, int64 with the leading axes kept (Python ints when there are none): an event is q >= thr, which for an integer q is
    q >= ceil(thr); a threshold above L - 1 gives no events, one <= 0 makes every pixel an event."""
    h = _counts(hist)
    L = h.shape[-1]
    thr = float(thr)
    if thr != thr:
        raise ValueError("joint_counts_at: the threshold is NaN")
    v = int(min(max(np.ceil(thr), 0), L))
    tp = h[..., v:, v:].sum(axis=(-2, -1))
    fn = h[..., v:, :v].sum(axis=(-2, -1))
    fp = h[..., :v, v:].sum(axis=(-2, -1))
    tn = h[..., :v, :v].sum(axis=(-2, -1))
    return tuple(_scalar(a) for a in (tp, fn, fp, tn))


def joint_entries(hist):
    """hist: (..., L, L) counts, the target's level on the row and the forecast's on the column -> the entries of done()["joint"], the
    leading axes (none, or T, or ops.joint_histogram's frames) kept in front of every array:
      "levels" L; "histogram" (L, L) int64; "marginal_target", "marginal_forecast" (L,) int64;
      "curves": per integer threshold v = 0 .. L - 1 the (L,) arrays TP, FN, FP, TN (int64, two-sided cumulative sums: TP[v] = sum of
                h[o >= v, f >= v]), CSI, POD, FAR, HSS (evaluator.contingency_metrics' formulas) and bias = (TP + FP) / (TP + FN);
      "conditional_mean" (L,): E[q_f | q_o = v], NaN where the target never took v;
      "qq" (L,) int64: the smallest u with CDF_o(u) >= CDF_f(v), the table that maps the forecast's marginal onto the observation's;
      "correlation": Pearson's r of (q_o, q_f) from the histogram's moments in float64, NaN when either variance is 0;
      "mean_error": E[q_f - q_o]."""
    h = _counts(hist)
    L = h.shape[-1]
    m_o, m_f = h.sum(axis=-1), h.sum(axis=-2)
    n = m_o.sum(axis=-1)
    tp = np.diagonal(_tail_sums(_tail_sums(h, -1), -2), axis1=-2, axis2=-1).copy()
    fn, fp = _tail_sums(m_o, -1) - tp, _tail_sums(m_f, -1) - tp
    tn = n[..., None] - tp - fn - fp
    as_f = [a.astype(np.float64) for a in (tp, fn, fp, tn)]
    metrics, all_far = contingency_metrics(as_f, (0,))
    level = np.arange(L, dtype=np.float64)
    nf = n.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        bias = (as_f[0] + as_f[2]) / (as_f[0] + as_f[1])
        cond = (h * level).sum(axis=-1) / m_o
        mean_o, mean_f = (m_o * level).sum(axis=-1) / nf, (m_f * level).sum(axis=-1) / nf
        d_o, d_f = level - mean_o[..., None], level - mean_f[..., None]
        var_o, var_f = (m_o * d_o * d_o).sum(axis=-1) / nf, (m_f * d_f * d_f).sum(axis=-1) / nf
        cov = (h * d_o[..., :, None] * d_f[..., None, :]).sum(axis=(-2, -1)) / nf
        corr = np.where((var_o > 0) & (var_f > 0), cov / np.sqrt(var_o * var_f), np.nan)
        mean_error = mean_f - mean_o
    cum_o, cum_f = np.cumsum(m_o, axis=-1), np.cumsum(m_f, axis=-1)
    qq = (cum_o[..., None, :] >= cum_f[..., :, None]).argmax(axis=-1).astype(np.int64)   # cum_o[L - 1] = n >= every cum_f: a True exists
    curves = {"TP": tp, "FN": fn, "FP": fp, "TN": tn, "CSI": metrics[0]["CSI"], "POD": metrics[0]["POD"], "FAR": all_far[0], "HSS": metrics[0]["HSS"],
              "bias": bias}
    return {"levels": L, "histogram": h, "marginal_target": m_o, "marginal_forecast": m_f, "curves": curves, "conditional_mean": cond, "qq": qq,
            "correlation": _scalar(corr), "mean_error": _scalar(mean_error)}


def object_entries(rows, frames, thresholds, min_area=1):
    """rows: (..., 2, nthr, ops.OBJ_COLS) integer sums (ops.object_stats' tensor, the Validator's table or its sum over the horizon; field 0 =
    target, 1 = forecast) and `frames`, the number of frames behind every row (samples for a row of the table, samples * T for the sum over
    the horizon) -> the entries of done()["objects"], the leading axes (none, or T) kept in front of every array:
      "min_area"; then per threshold key
        "target", "forecast": "count" N, "per_frame" N / frames, "area" sum a, "mean_area" sum a / N, "weighted_area" sum a^2 / sum a (the
            size of the object a random event pixel lies in), "mean_largest" (the largest object's area, a frame without objects counting
            0), "matched" (objects with a pixel that is an event of the other field), "matched_area", "size_histogram" (17 int64: objects
            with floor(log2(area)) = k);
        "count_bias" N_f / N_o, "size_bias" weighted_area_f / weighted_area_o, "object_POD" matched_o / N_o, "object_FAR"
            1 - matched_f / N_f, "object_CSI" matched_o / (N_o + N_f - matched_f), "size_bin_edges" 2^k.
    A division by zero gives NaN."""
    if torch.is_tensor(rows):
        rows = rows.detach().cpu().numpy()
    r = np.asarray(rows)
    nthr = len(thresholds)
    if r.ndim < 3 or r.shape[-3:] != (2, nthr, ops.OBJ_COLS):
        raise ValueError(f"objects: rows are (..., 2, {nthr}, {ops.OBJ_COLS}) for {nthr} thresholds, got {r.shape}")
    if r.dtype.kind == "f":
        if not (np.isfinite(r).all() and (r == np.rint(r)).all()):
            raise ValueError("objects: the rows hold integer sums")
    elif r.dtype.kind not in "iu":
        raise ValueError(f"objects: the rows hold integer sums, got {r.dtype}")
    r = r.astype(np.int64)
    frames = np.asarray(frames, dtype=np.float64)

    def ratio(a, b):
        """a / b in float64, NaN where b is 0"""
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return _scalar(np.where(b == 0, np.nan, a / b))

    def field(c):
        n, a, a2, big, m, ma = (c[..., i] for i in range(6))
        return {"count": _scalar(n), "per_frame": ratio(n, frames), "area": _scalar(a), "mean_area": ratio(a, n), "weighted_area": ratio(a2, a),
                "mean_largest": ratio(big, frames), "matched": _scalar(m), "matched_area": _scalar(ma), "size_histogram": c[..., 6:].copy()}
    res = {"min_area": int(min_area)}
    for k, thr in enumerate(thresholds):
        o, f = field(r[..., 0, k, :]), field(r[..., 1, k, :])
        res[_thr_key(thr)] = {"target": o, "forecast": f, "count_bias": ratio(f["count"], o["count"]),
                              "size_bias": ratio(f["weighted_area"], o["weighted_area"]), "object_POD": ratio(o["matched"], o["count"]),
                              "object_FAR": 1.0 - ratio(f["matched"], f["count"]),
                              "object_CSI": ratio(o["matched"], np.asarray(o["count"]) + f["count"] - f["matched"]),
                              "size_bin_edges": 2 ** np.arange(ops.OBJ_BINS, dtype=np.int64)}
    return res


def sal_entries(rows, thresholds, spec=(1, None)):
    """rows: (..., nthr, ops.SAL_COLS) sums (the Validator's table, its sum over the horizon, or a sum of ops.sal_table's rows) and spec =
    (min_area, intensity) as ops.sal_spec returns it -> the entries of done()["sal"], the leading axes (none, or T) kept in front of every
    array:
      "min_area", "intensity" (the table as a tuple, None for the identity); then per threshold key
        "A", "abs_A" (means over "frames_A", the frames where either field has mass), "S", "abs_S", "L2", "L" (means over "frames_S", the
        frames where both fields have an object), "L1" (mean over "frames_L1", the frames where both fields have mass), and "frames_A",
        "frames_L1", "frames_S", "missed_frames" (only the target has an object), "false_frames" (only the forecast has one).
    A mean over no frame is NaN."""
    if torch.is_tensor(rows):
        rows = rows.detach().cpu().numpy()
    r = np.asarray(rows, dtype=np.float64)
    nthr = len(thresholds)
    if r.ndim < 2 or r.shape[-2:] != (nthr, ops.SAL_COLS):
        raise ValueError(f"sal: rows are (..., {nthr}, {ops.SAL_COLS}) for {nthr} thresholds, got {r.shape}")
    counts = r[..., [0, 3, 5, 10, 11]]
    if not (np.isfinite(counts).all() and (counts == np.rint(counts)).all() and (counts >= 0).all()):
        raise ValueError("sal: columns 0, 3, 5, 10 and 11 of the rows hold frame counts")
    min_area, intensity = spec

    def mean(col, count):
        with np.errstate(divide="ignore", invalid="ignore"):
            return _scalar(np.where(count == 0, np.nan, col / count))

    def count(col):
        return _scalar(col.astype(np.int64))
    res = {"min_area": int(min_area), "intensity": None if intensity is None else tuple(intensity)}
    for k, thr in enumerate(thresholds):
        c = r[..., k, :]
        n_a, n_l1, n_s = c[..., 0], c[..., 3], c[..., 5]
        res[_thr_key(thr)] = {"A": mean(c[..., 1], n_a), "abs_A": mean(c[..., 2], n_a), "S": mean(c[..., 6], n_s), "abs_S": mean(c[..., 7], n_s),
                              "L1": mean(c[..., 4], n_l1), "L2": mean(c[..., 8], n_s), "L": mean(c[..., 9], n_s), "frames_A": count(n_a),
                              "frames_L1": count(n_l1), "frames_S": count(n_s), "missed_frames": count(c[..., 10]), "false_frames": count(c[..., 11])}
    return res


def _ratio(a, b):
    """a / b in float64, NaN where b is 0"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return _scalar(np.where(b == 0, np.nan, a / b))


def _probability_entry(n0, n1, m, bins):
    """n0, n1: (..., m + 1) counts of the pixels without / with the observed event per forecast count c = 0 .. m, the forecast being
    p = c / m (m = n^2 window pixels for nprob_entries, m = M members for ensemble_entries) -> the verification of that discrete
    probability forecast, as nprob_entries states it"""
    ratio = _ratio
    c = np.arange(m + 1)
    p = c / float(m)
    both = (n0 + n1).astype(np.float64)
    total, events, quiet = both.sum(axis=-1), n1.sum(axis=-1), n0.sum(axis=-1)
    base = np.asarray(ratio(events, total))
    freq = np.asarray(ratio(n1, both))   # the observed frequency given the forecast value; NaN where the value never occurs
    rel = np.where(both == 0, 0.0, both * (p - freq) ** 2).sum(axis=-1)
    res = np.where(both == 0, 0.0, both * (freq - base[..., None]) ** 2).sum(axis=-1)
    brier, unc = np.asarray(ratio((n0 * p ** 2 + n1 * (p - 1.0) ** 2).sum(axis=-1), total)), base * (1.0 - base)
    zero = np.zeros(n0.shape[:-1] + (1,))
    pod = np.concatenate([np.asarray(ratio(_tail_sums(n1, -1), events[..., None])), zero], axis=-1)
    pofd = np.concatenate([np.asarray(ratio(_tail_sums(n0, -1), quiet[..., None])), zero], axis=-1)
    area = ((pofd[..., :-1] - pofd[..., 1:]) * (pod[..., :-1] + pod[..., 1:]) / 2.0).sum(axis=-1)
    member = (np.minimum(c * bins // m, bins - 1)[:, None] == np.arange(bins)).astype(np.float64)   # (m + 1, bins), one bin per value
    count = both @ member
    return {"histogram": np.stack([n0, n1], axis=-2), "base_rate": _scalar(base), "brier": _scalar(brier),
            "reliability": ratio(rel, total), "resolution": ratio(res, total), "uncertainty": _scalar(unc),
            "brier_skill": _scalar(1.0 - np.asarray(ratio(brier, unc))), "roc": {"pofd": pofd, "pod": pod}, "roc_area": _scalar(area),
            "reliability_diagram": {"edges": np.linspace(0.0, 1.0, bins + 1), "count": count.astype(np.int64),
                                    "forecast_mean": ratio((both * p) @ member, count), "observed_frequency": ratio(n1.astype(np.float64) @ member, count)}}


def ensemble_entries(rows, M, thresholds, bins=10):
    """rows: (..., C) integer sums laid out as ops.ensemble_cols(M, nthr) states (ops.ensemble_table's tensor summed over its frames, the
    Validator's table or its sum over the horizon) -> the entries of done()["ensemble"], the leading axes (none, or T) kept in front of every
    array.  Every level is in units of q, the quantised value floor(clip(v, 0, 1) * value_scale), NOT in the model's units.  With N pixels,
    y the target's level and x_i the members':
      "members" M, "pixels" N, "dry" Z (the pixels where the target and every member are 0);
      "crps" S1 / (M N) - S2 / (M^2 N), the CRPS of the ensemble's empirical distribution; "crps_fair" with M (M - 1) in the second term
        (Ferro's fair CRPS, NaN-free for M >= 2); "mae_control" S0 / N, the CRPS of the deterministic control (member 0) and so the skill's
        zero; "crpss" 1 - crps / mae_control;
      "spread" sqrt(V / (M (M - 1) N)), the root of the mean unbiased member variance; "rmse_mean" sqrt(E / (M^2 N)), the RMSE of the ensemble
        mean; "spread_skill" sqrt((M + 1) / M) spread / rmse_mean (1 for a statistically consistent ensemble);
      "rank_histogram" (M + 1) float64: the target's rank among the members, the ties of a pixel with b members below and e equal shared
        equally among the ranks b .. b + e (the dry pixels are such ties: each adds 1 / (M + 1) to every rank); "rank_histogram_wet": the
        same without the dry pixels;
      per threshold key: the entry nprob_entries forms, from the counts of the pixels without / with the observed event per number c of
        members at or above the threshold, the forecast being p = c / M: "histogram" (2, M + 1), "base_rate", "brier", "reliability",
        "resolution", "uncertainty", "brier_skill", "roc", "roc_area", "reliability_diagram".
    The table keeps the dry pixels in Z alone (include/adnm_hip.h); they are put back here: into rank bin (0, M), and per threshold into
    (o = 0, c = 0), or for a threshold <= 0, where every pixel is an event, into (o = 1, c = M).  A division by zero gives NaN."""
    if torch.is_tensor(rows):
        rows = rows.detach().cpu().numpy()
    r = np.asarray(rows)
    M, nthr, bins = int(M), len(thresholds), int(bins)
    C, at = ops.ensemble_cols(M, nthr)   # ValueError outside the limits
    if r.ndim < 1 or r.shape[-1] != C:
        raise ValueError(f"ensemble: rows are (..., {C}) for {M} members and {nthr} thresholds, got {r.shape}")
    if bins < 1:
        raise ValueError(f"ensemble: bins >= 1, got {bins}")
    if r.dtype.kind == "f":
        if not (np.isfinite(r).all() and (r == np.rint(r)).all()):
            raise ValueError("ensemble: the rows hold integer sums")
    elif r.dtype.kind not in "iu":
        raise ValueError(f"ensemble: the rows hold integer sums, got {r.dtype}")
    r = r.astype(np.int64)
    if (r < 0).any():
        raise ValueError("ensemble: the rows hold sums >= 0")
    n, z, s0, s1, s2, v, e = (r[..., i].astype(np.float64) for i in range(7))
    fm = float(M)
    crps = np.asarray(_ratio(s1, fm * n)) - np.asarray(_ratio(s2, fm * fm * n))
    fair = np.asarray(_ratio(s1, fm * n)) - np.asarray(_ratio(s2, fm * (fm - 1.0) * n))
    mae = np.asarray(_ratio(s0, n))
    spread, rmse = np.sqrt(np.asarray(_ratio(v, fm * (fm - 1.0) * n))), np.sqrt(np.asarray(_ratio(e, fm * fm * n)))
    # ties: bin (b, e) gives 1 / (e + 1) to each of the ranks b .. b + e
    bins_r = r[..., at["rank"]:at["rank"] + (M + 1) ** 2].reshape(r.shape[:-1] + (M + 1, M + 1)).astype(np.float64)
    share = np.zeros((M + 1, M + 1, M + 1))
    for b in range(M + 1):
        for eq in range(M + 1 - b):
            share[b, eq, b:b + eq + 1] = 1.0 / (eq + 1)
    wet = np.einsum("...be,ber->...r", bins_r, share)
    res = {"members": M, "pixels": _scalar(r[..., 0]), "dry": _scalar(r[..., 1]), "crps": _scalar(crps), "crps_fair": _scalar(fair), "mae_control": _scalar(mae),
           "crpss": _scalar(1.0 - np.asarray(_ratio(crps, mae))), "spread": _scalar(spread), "rmse_mean": _scalar(rmse),
           "spread_skill": _scalar(math.sqrt((fm + 1.0) / fm) * np.asarray(_ratio(spread, rmse))),
           "rank_histogram": wet + z[..., None] / (fm + 1.0), "rank_histogram_wet": wet}
    for k, thr in enumerate(thresholds):
        a = at["exceed"] + 2 * k * (M + 1)
        n0, n1 = r[..., a:a + M + 1].copy(), r[..., a + M + 1:a + 2 * (M + 1)].copy()
        if float(thr) <= 0.0:
            n1[..., M] += r[..., 1]
        else:
            n0[..., 0] += r[..., 1]
        res[_thr_key(thr)] = _probability_entry(n0, n1, M, bins)
    return res


def nprob_entries(rows, scales, thresholds, bins=10):
    """rows: (..., nthr, S) integer counts laid out as ops.nprob_layout(scales) states (ops.neighbour_hist's tensor summed over its frames, the
    Validator's table or its sum over the horizon) -> the entries of done()["nprob"], {n: {thr: {...}}}, the leading axes (none, or T) kept
    in front of every array.  The forecast is p = c / n^2, c = 0 .. n^2, the observation o the event bit at the pixel; N = the counts:
      "histogram" int64 (2, n^2 + 1), [o][c]; "base_rate" SUM N[1] / SUM N;
      "brier" SUM N (p - o)^2 / SUM N; "reliability", "resolution", "uncertainty": Murphy's decomposition over the n^2 + 1 distinct forecast
        values (exact for this discrete forecast: brier = reliability - resolution + uncertainty); "brier_skill" 1 - brier / uncertainty;
      "roc" {"pofd", "pod"}: the decision "warn when c >= c*" for c* = 0 .. n^2, then the point (0, 0): n^2 + 2 points from (1, 1) down;
        "roc_area" the trapezoid under them;
      "reliability_diagram" {"edges" (bins + 1), "count", "forecast_mean", "observed_frequency" (bins)}: equal-width bins of p, bin b holding
        b / bins <= p < (b + 1) / bins (compared in integers), the last one closed on the right.
    A division by zero gives NaN."""
    if torch.is_tensor(rows):
        rows = rows.detach().cpu().numpy()
    r = np.asarray(rows)
    scales, nthr, bins = ops.fss_scales(scales), len(thresholds), int(bins)
    layout, S = ops.nprob_layout(scales)
    if not scales or r.ndim < 2 or r.shape[-2:] != (nthr, S):
        raise ValueError(f"nprob: rows are (..., {nthr}, {S}) for {nthr} thresholds and scales {scales}, got {r.shape}")
    if bins < 1:
        raise ValueError(f"nprob: bins >= 1, got {bins}")
    if r.dtype.kind == "f":
        if not (np.isfinite(r).all() and (r == np.rint(r)).all()):
            raise ValueError("nprob: the rows hold integer counts")
    elif r.dtype.kind not in "iu":
        raise ValueError(f"nprob: the rows hold integer counts, got {r.dtype}")
    r = r.astype(np.int64)

    return {n: {_thr_key(thr): _probability_entry(r[..., k, a0:a0 + n * n + 1], r[..., k, a1:a1 + n * n + 1], n * n, bins) for k, thr in enumerate(thresholds)}
            for n, (a0, a1) in zip(scales, layout)}


def track_entries(rows, samples, thresholds, T, min_volume=1):
    """rows: (2, nthr, 7 + 4 T) integer sums (ops.track_stats' tensor summed over its samples, or the Validator's table; field 0 = target,
    1 = forecast; columns: ops.track_cols) and `samples`, the number of samples behind them -> the entries of done()["tracks"]:
      "min_volume"; then per threshold key
        "target", "forecast": "count" N, "per_sample" N / samples, "volume" sum v, "mean_volume" sum v / N, "weighted_volume" sum v^2 / sum v
            (the volume of the track a random event voxel lies in), "mean_duration" sum d / N, "duration_histogram" (T int64: tracks of d = k + 1
            frames), "births", "deaths" (T int64: tracks by first / last frame), "alive" (T int64: alive[t] = births up to t minus deaths
            before t), "initial" births[0], "survival" (T: the share of the initial tracks whose last frame is t or later; NaN without
            initial tracks), "spanning" (first frame 0 and last frame T - 1), "matched" (tracks with a voxel that is an event of the other
            field), "matched_volume";
        "count_bias" N_f / N_o, "duration_bias" mean_duration_f / mean_duration_o, "survival_bias" survival_f / survival_o per frame index,
            "track_POD" matched_o / N_o, "track_FAR" 1 - matched_f / N_f, "track_CSI" matched_o / (N_o + N_f - matched_f).
    A division by zero gives NaN.  Every array is per lead time already: a track belongs to no single frame index."""
    if torch.is_tensor(rows):
        rows = rows.detach().cpu().numpy()
    r = np.asarray(rows)
    nthr, (C, at) = len(thresholds), ops.track_cols(T)
    T = int(T)
    if r.shape != (2, nthr, C):
        raise ValueError(f"tracks: rows are (2, {nthr}, {C}) for {nthr} thresholds and T = {T}, got {r.shape}")
    if r.dtype.kind == "f":
        if not (np.isfinite(r).all() and (r == np.rint(r)).all()):
            raise ValueError("tracks: the rows hold integer sums")
    elif r.dtype.kind not in "iu":
        raise ValueError(f"tracks: the rows hold integer sums, got {r.dtype}")
    r = r.astype(np.int64)

    def ratio(a, b):
        """a / b in float64, NaN where b is 0"""
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return _scalar(np.where(b == 0, np.nan, a / b))

    def field(c):
        n, v, v2, d, m, mv, span = (int(c[i]) for i in range(7))
        births, deaths, deaths0, hist = (c[at[k]:at[k] + T].copy() for k in ("births", "deaths", "deaths0", "duration_histogram"))
        alive = np.cumsum(births) - (np.cumsum(deaths) - deaths)
        return {"count": n, "per_sample": ratio(n, samples), "volume": v, "mean_volume": ratio(v, n), "weighted_volume": ratio(v2, v),
                "mean_duration": ratio(d, n), "duration_histogram": hist, "births": births, "deaths": deaths, "alive": alive,
                "initial": int(births[0]), "survival": ratio(_tail_sums(deaths0, -1), np.full(T, births[0])), "spanning": span, "matched": m,
                "matched_volume": mv}
    res = {"min_volume": int(min_volume)}
    for k, thr in enumerate(thresholds):
        o, f = field(r[0, k]), field(r[1, k])
        res[_thr_key(thr)] = {"target": o, "forecast": f, "count_bias": ratio(f["count"], o["count"]),
                              "duration_bias": ratio(f["mean_duration"], o["mean_duration"]), "survival_bias": ratio(f["survival"], o["survival"]),
                              "track_POD": ratio(o["matched"], o["count"]), "track_FAR": 1.0 - ratio(f["matched"], f["count"]),
                              "track_CSI": ratio(o["matched"], o["count"] + f["count"] - f["matched"])}
    return res


def intensity_scale_entries(rows, frames, shape, thresholds):
    """rows: (..., L + 1, 3 * nthr) integer sums A, F, C per level and threshold (ops.intensity_scale_sums' tensor summed over its frames, the
    Validator's table or its sum over the horizon), `frames` the number n of frames behind every row (samples for a row of the table,
    samples * T for the sum over the horizon) and shape = (H, W) of the frames -> the entries of done()["intensity_scale"], the leading axes
    (none, or T) kept in front of every array.  (P, L) = ops.intensity_scale_levels(H, W), N = n P^2, D_l = A_l + F_l - 2 C_l and
    E_l(X) = X_l / (4^l N), the mean square of the field of block means:
      "scale_px" 2^j for j = 0 .. L (int64), "domain_px" P, "levels" L; then per threshold key
        "mse" (L + 1): E_j(D) - E_(j+1)(D) for j < L and E_L(D) for the domain mean, the MSE of the Haar component of scale 2^j of the binary
            error; formed as (4 D_j - D_(j+1)) / (4^(j+1) N) with the numerator in integers, so a component is never below 0;
        "mse_total" D_0 / N = (FP + FN) / N (the components sum to it), "mse_share" mse / mse_total;
        "base_rate" e = A_0 / N, "bias" B = F_0 / A_0, "mse_random" B e (1 - e) + e (1 - B e) (a random forecast of the same bias; 2 e (1 - e)
            when unbiased: Casati 2004);
        "skill" 1 - mse (L + 1) / mse_random (its mean over the scales is 1 - mse_total / mse_random);
        "energy_target", "energy_forecast" (L + 1): the same split of A and of F (they sum to e and to B e);
        "energy_rel_diff" (En_f - En_o) / (En_f + En_o).
    A division by zero gives NaN."""
    if torch.is_tensor(rows):
        rows = rows.detach().cpu().numpy()
    r = np.asarray(rows)
    P, L = ops.intensity_scale_levels(*shape)
    nthr = len(thresholds)
    if r.ndim < 2 or r.shape[-2:] != (L + 1, 3 * nthr):
        raise ValueError(f"intensity_scale: rows are (..., {L + 1}, {3 * nthr}) for {nthr} thresholds and frames of {shape[0]} x {shape[1]}, got {r.shape}")
    if r.dtype.kind == "f":
        if not (np.isfinite(r).all() and (r == np.rint(r)).all()):
            raise ValueError("intensity_scale: the rows hold integer sums")
    elif r.dtype.kind not in "iu":
        raise ValueError(f"intensity_scale: the rows hold integer sums, got {r.dtype}")
    r = r.astype(np.int64)
    if (r < 0).any():
        raise ValueError("intensity_scale: the rows hold sums >= 0")
    N = np.asarray(frames, dtype=np.float64)[..., None] * float(P * P)      # (..., 1): broadcasts over the levels
    if N.ndim > r.ndim - 1:
        raise ValueError(f"intensity_scale: frames {np.shape(frames)} do not fit rows {r.shape}")
    four = 4.0 ** np.arange(L + 1)

    def ratio(a, b):
        """a / b in float64, NaN where b is 0"""
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(b == 0, np.nan, a / b)

    def split(x):
        """(..., L + 1) integer sums X_l -> (..., L + 1) E_j(X) - E_(j+1)(X), the last one E_L(X)"""
        num = 4 * x
        num[..., :-1] -= x[..., 1:]
        return ratio(num, 4.0 * four * N)
    res = {"scale_px": 2 ** np.arange(L + 1, dtype=np.int64), "domain_px": P, "levels": L}
    for k, thr in enumerate(thresholds):
        a, f, c = r[..., 3 * k], r[..., 3 * k + 1], r[..., 3 * k + 2]
        d = a + f - 2 * c
        mse, en_o, en_f = split(d), split(a), split(f)
        total, base, bias = ratio(d[..., :1], N), ratio(a[..., :1], N), ratio(f[..., :1], a[..., :1])      # (..., 1)
        rand = bias * base * (1.0 - base) + base * (1.0 - bias * base)
        res[_thr_key(thr)] = {"mse": mse, "skill": 1.0 - ratio(mse * (L + 1), rand), "mse_share": ratio(mse, total), "mse_total": _scalar(total[..., 0]),
                              "mse_random": _scalar(rand[..., 0]), "base_rate": _scalar(base[..., 0]), "bias": _scalar(bias[..., 0]),
                              "energy_target": en_o, "energy_forecast": en_f, "energy_rel_diff": ratio(en_f - en_o, en_f + en_o)}
    return res


def _spectrum_entries(sums, cells, wavelength):
    """(..., R, 3) sums P_o, P_f, C and the (..., R)-broadcastable number of coefficients behind each -> the entries of "spectrum"; the
    leading axes (none, or T) are kept"""
    sums = np.asarray(sums, dtype=np.float64)
    p_o, p_f, c = sums[..., 0], sums[..., 1], sums[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = p_f / p_o
        coherence = np.where((p_o == 0) | (p_f == 0), np.nan, c / np.sqrt(p_o * p_f))
        target, forecast = p_o / cells, p_f / cells
    keeps = np.cumprod(ratio[..., 1:] >= 0.5, axis=-1).sum(axis=-1)   # the largest r with ratio >= 0.5 at every bin 1 .. r (0: bin 1 fails)
    eff = np.where(keeps > 0, wavelength[keeps], np.inf)
    return {"wavenumber": np.arange(sums.shape[-2]), "wavelength_px": wavelength, "target": target, "forecast": forecast, "ratio": ratio,
            "coherence": coherence, "effective_resolution_px": float(eff) if eff.ndim == 0 else eff}


def _fss(sums):
    """(..., 3 * nthr) sums A, F, C -> (..., nthr) FSS = 2C / (A + F); NaN where A + F = 0 (no event in either field)"""
    sums = np.asarray(sums, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 * sums[..., 2::3] / (sums[..., 0::3] + sums[..., 1::3])


def _thr_key(thr):
    """the key contingency_metrics gives a threshold"""
    return int(thr) if float(thr).is_integer() else thr


def _fss_scores(tab, scales, thresholds):
    """(T, nscale, 3 * nthr) -> {n: {thr: FSS over the horizon}}"""
    score = _fss(tab.sum(axis=0))
    return {n: {_thr_key(thr): float(score[i, k]) for k, thr in enumerate(thresholds)} for i, n in enumerate(scales)}


def _fss_lead(tab, scales, thresholds):
    """(T, nscale, 3 * nthr) -> {n: {thr: length-T array of FSS per frame index}}"""
    score = _fss(tab)
    return {n: {_thr_key(thr): score[:, i, k].copy() for k, thr in enumerate(thresholds)} for i, n in enumerate(scales)}


def _scores(counts, thresholds):
    """(4 * nthr) counts summed over the horizon -> the two entries every scored field has"""
    metrics, all_far = contingency_metrics(counts, thresholds)
    return {"threshold_metrics": metrics, "FAR": float(np.mean(all_far))}


def _lead_scores(rows, thresholds):
    """(T, 4 * nthr) counts per frame index -> {thr: {TP, TN, FP, FN, CSI, POD, HSS, FAR}}, each a length-T array: contingency_metrics'
    formulas applied to the rows (its sums[4k:4k+4] are then four length-T arrays)"""
    metrics, all_far = contingency_metrics(rows.T, thresholds)
    for m, far in zip(metrics.values(), all_far):
        m["FAR"] = far
    return metrics


def aggregate(block, thresholds, seq_len, hw, ssim_area, pools=(), persistence=False, per_lead=False, fss=(), advection=False, spectrum=None,
              sal=None, nprob=None, tracks=None, intensity_scale=None, ensemble=None, objects=None, joint=None):
    """host: the block (a float64 array laid out as block_layout states for these options; `spectrum` = (H, W), the frame size, `joint` = L,
    the number of levels: include/adnm_hip.h) -> the dictionary of Validator.done().  The metrics are SimplifiedEvaluator.done's
    (Shanghai_metrics.py:218-290) as GpuEvaluator.done() states them, from per-frame-index sums; "pooled", "persistence", "advection" and
    "per_lead" apply the same formulas to the pooled tables, the baselines' tables and the single rows.  `fss`: "fss" {n: {thr: 2C / (A + F)}},
    also under each baseline and under "per_lead", and "fss_useful" {thr: 0.5 + f_o / 2} with f_o the observed event fraction of the main
    table (the line above which a scale is called useful).  `spectrum`: "spectrum" {"wavenumber", "wavelength_px", "target" and "forecast"
    (mean power per coefficient: sum / (n_r * samples * T)), "ratio" (forecast / target), "coherence" (C / sqrt(P_o P_f) of the sums over the
    horizon, NaN where a power is 0), "effective_resolution_px" (the wavelength of the largest r >= 1 with ratio >= 0.5 at every bin 1 .. r;
    inf when bin 1 fails)}, and under "per_lead" the same as (T, R) arrays from the single rows.  `joint`: "joint" = joint_entries of the
    histogram's sum over the horizon, and under "per_lead" joint_entries of the table, every array with a leading T axis.  `objects` (what
    ops.objects_spec takes): "objects" = object_entries of the table's sum over the horizon, and under "per_lead" object_entries of the table.
    `sal` (what ops.sal_spec takes; passed BY NAME, its position in front of `objects` is not part of the interface): "sal" = sal_entries of the
    table's sum over the horizon, and under "per_lead" sal_entries of the table.  `nprob` (the scales; BY NAME): "nprob" = nprob_entries of the
    table's sum over the horizon, and under "per_lead" nprob_entries of the table.  `tracks` (what ops.tracks_spec takes; BY NAME): "tracks" =
    track_entries of the table.  Its arrays are per lead time already, so per_lead=True adds nothing for tracks.  `intensity_scale` ((H, W), the
    frame size; BY NAME): "intensity_scale" = intensity_scale_entries of the table's sum over the horizon, the same under each baseline there
    is, and under "per_lead" intensity_scale_entries of the tables.  `ensemble` (the number of members M; BY NAME): "ensemble" =
    ensemble_entries of the table's sum over the horizon, and under "per_lead" ensemble_entries of the table."""
    nthr, T = len(thresholds), seq_len
    pools, fss = tuple(pools), tuple(fss)
    spectrum = tuple(int(v) for v in spectrum) if spectrum else None
    if spectrum:
        n_r, wavelength = ops.spectrum_bins(*spectrum)   # ValueError outside the limits
    joint = int(joint) if joint else None
    if joint is not None and not ops.MIN_JOINT_LEVELS <= joint <= ops.MAX_JOINT_LEVELS:
        raise ValueError(f"aggregate: joint is the number of levels, {ops.MIN_JOINT_LEVELS}..{ops.MAX_JOINT_LEVELS}, or None; got {joint}")
    objects, sal, nprob, tracks = ops.objects_spec(objects), ops.sal_spec(sal), ops.fss_scales(nprob), ops.tracks_spec(tracks)
    iscale = tuple(int(v) for v in intensity_scale) if intensity_scale else None
    ensemble = int(ensemble) if ensemble else None
    parts, total = block_rows(T, nthr, pools, persistence, fss, advection, spectrum, joint, sal=sal, nprob=nprob, tracks=tracks, objects=objects,
                              iscale=iscale, ensemble=ensemble)   # ValueError outside the intensity-scale limits
    blk = np.asarray(block, dtype=np.float64)
    if blk.shape != (total,):
        raise ValueError(f"aggregate: a block of {total} doubles is expected for {T} frames, {nthr} thresholds, pools {pools}, "
                         f"persistence {bool(persistence)}" + (f", fss {fss}" if fss else "") + (", advection" if advection else "")
                         + (f", spectrum of {spectrum[0]} x {spectrum[1]} frames" if spectrum else "") + (f", a joint histogram of {joint} levels" if joint else "")
                         + (", objects" if objects else "") + (", sal" if sal else "") + (f", nprob {nprob}" if nprob else "")
                         + (f", intensity_scale of {iscale[0]} x {iscale[1]} frames" if iscale else "") + (f", an ensemble of {ensemble}" if ensemble else "") + (", tracks" if tracks else "") + f"; got {blk.shape}")
    tabs = {p.name: blk[p.offset:p.offset + p.size].reshape(p.shape) for p in parts}
    loss_sum, batches, samples, nonfinite = (float(v) for v in blk[:HEADER])
    tab = tabs["main"][HEADER:].reshape(T, 4 * nthr + 3)
    cells = tab[:, :4 * nthr].sum(axis=0)
    metrics, all_far = contingency_metrics(cells, thresholds)
    with np.errstate(divide="ignore", invalid="ignore"):
        mse_t = tab[:, 4 * nthr + 1] / (hw * samples)            # per frame index: the mean over the samples of the frame's MSE
        rmse = float(np.mean(np.sqrt(mse_t)))
        mae = float(tab[:, 4 * nthr].sum() / (hw * samples * T))
        ssim = None if ssim_area is None else float(tab[:, 4 * nthr + 2].sum() / (ssim_area * samples * T))
        finite = batches - nonfinite
    res = {"threshold_metrics": metrics, "FAR": float(np.mean(all_far)), "RMSE": rmse, "MAE": mae, "MSE": float(mse_t.mean()), "SSIM": ssim,
           "LPIPS": None, "loss_sum": loss_sum, "loss_mean": loss_sum / finite if finite > 0 else float("nan"), "batches": int(batches),
           "samples": int(samples), "nonfinite": int(nonfinite)}

    def counted(rows, lead):
        """(T, 4 * nthr) counts of one field at one pool -> its entries over the horizon, or per frame index"""
        return {"threshold_metrics": _lead_scores(rows, thresholds)} if lead else _scores(rows.sum(axis=0), thresholds)

    def baseline(name, lead):
        """the entries of a baseline field (persistence, advection) from its pooled table and, with fss, its FSS table"""
        rows, order = tabs[name + "/pooled"], baseline_pools(pools)
        ent = dict(counted(rows[:, 0], lead), pooled={p: counted(rows[:, order.index(p)], lead) for p in pools})
        if fss:
            ent["fss"] = (_fss_lead if lead else _fss_scores)(tabs[name + "/fss"], fss, thresholds)
        if iscale:
            ent["intensity_scale"] = scales(tabs[name + "/iscale"], lead)
        return ent

    def scales(itab, lead):
        """(T, L + 1, 3 * nthr) intensity-scale sums of one field -> its entries over the horizon, or per frame index"""
        return intensity_scale_entries(itab if lead else itab.sum(axis=0), samples if lead else samples * T, iscale, thresholds)

    def optional(lead):
        """the entries the options add, in the dictionary's order: over the horizon, or (lead) per frame index"""
        if pools:
            yield "pooled", {p: counted(tabs["pooled"][:, i], lead) for i, p in enumerate(pools)}
        if persistence:
            yield "persistence", baseline("persistence", lead)
        if fss:
            yield "fss", (_fss_lead if lead else _fss_scores)(tabs["fss"], fss, thresholds)
            if not lead:
                with np.errstate(divide="ignore", invalid="ignore"):
                    yield "fss_useful", {_thr_key(thr): float(0.5 + (cells[4 * k] + cells[4 * k + 1]) / cells[4 * k:4 * k + 4].sum() / 2.0)
                                         for k, thr in enumerate(thresholds)}
        if advection:
            yield "advection", baseline("advection", lead)
        if spectrum:
            stab = tabs["spectrum"]
            yield "spectrum", _spectrum_entries(stab if lead else stab.sum(axis=0), n_r * (samples if lead else samples * T), wavelength)
        if joint:
            yield "joint", joint_entries(tabs["joint"] if lead else tabs["joint"].sum(axis=0))
        if objects:
            otab = tabs["objects"]
            yield "objects", object_entries(otab if lead else otab.sum(axis=0), samples if lead else samples * T, thresholds, objects)
        if sal:
            yield "sal", sal_entries(tabs["sal"] if lead else tabs["sal"].sum(axis=0), thresholds, sal)
        if nprob:
            yield "nprob", nprob_entries(tabs["nprob"] if lead else tabs["nprob"].sum(axis=0), nprob, thresholds)
        if iscale:
            yield "intensity_scale", scales(tabs["iscale"], lead)
        if ensemble:
            yield "ensemble", ensemble_entries(tabs["ensemble"] if lead else tabs["ensemble"].sum(axis=0), ensemble, thresholds)
        if tracks and not lead:
            yield "tracks", track_entries(tabs["tracks"], samples, thresholds, T, tracks)
    res.update(optional(False))
    if per_lead:
        with np.errstate(divide="ignore", invalid="ignore"):
            lead = {"RMSE": np.sqrt(mse_t), "MAE": tab[:, 4 * nthr] / (hw * samples),
                    "SSIM": None if ssim_area is None else tab[:, 4 * nthr + 2] / (ssim_area * samples),
                    "threshold_metrics": _lead_scores(tab[:, :4 * nthr], thresholds)}
        lead.update(optional(True))
        res["per_lead"] = lead
    return res


class Validator(ForwardClient):
    def __init__(self, model, loss_fn, seq_len, value_scale, thresholds=(20, 30, 35, 40), ssim=True, process_group=None, pools=None, persistence=False,
                 fss=None, advection=None, spectrum=False, objects=None, advection_flow=False, sal=None, nprob=None, tracks=None, intensity_scale=False,
                 ensemble=None, joint=False):
        from models.loss import enRainfallLoss
        if not isinstance(loss_fn, enRainfallLoss):   # RainfallLoss is a subclass
            raise RuntimeError(f"Validator: loss_fn must be an enRainfallLoss / RainfallLoss (the loss csrc/dataio.hip::valid_accum computes; "
                               f"there is no torch fallback), got {type(loss_fn).__name__}")
        self.model, self.loss_fn, self.seq_len, self.value_scale = model, loss_fn, int(seq_len), float(value_scale)
        self.thresholds = [float(t) for t in thresholds]
        if not 1 <= len(self.thresholds) <= 8:
            raise ValueError("1..8 thresholds")
        if self.seq_len < 1:
            raise ValueError("seq_len >= 1")
        self.ssim, self.process_group = bool(ssim), process_group
        self.pools, self.persistence = ops.pool_pairs(pools), bool(persistence)   # (size, stride) pairs; ValueError on a bad entry
        self.fss = ops.fss_scales(fss)   # distinct odd scales <= 33; ValueError on a bad entry
        self.advection = ops.advection_spec(advection, self.thresholds)   # (block, radius, echo) or None; ValueError on a bad entry
        if self.advection and not 0.0 < self.value_scale <= 255.0:
            raise ValueError(f"Validator: advection matches blocks on quantised bytes, which needs 0 < value_scale <= 255, got {self.value_scale}")
        self.advection_flow = bool(advection_flow)   # the advected field by sub-pixel flow and transport along it (csrc/flow.hip) instead of block copies
        if self.advection_flow and not self.advection:
            raise ValueError("Validator: advection_flow=True chooses how the advection baseline moves the frame; it needs advection= as well")
        if self.advection_flow and self.seq_len > ops.MAX_FLOW_T:
            raise ValueError(f"Validator: advection_flow follows a displacement in int32, which needs seq_len <= {ops.MAX_FLOW_T}, got {self.seq_len}")
        self.spectrum, self.joint = bool(spectrum), bool(joint)
        self._levels = ops.joint_levels(self.value_scale) if self.joint else None   # ValueError outside the limits
        self.objects = ops.objects_spec(objects)   # min_area, or None; ValueError on a bad entry
        self.sal = ops.sal_spec(sal)   # (min_area, intensity), or None; ValueError on a bad entry
        self._weights = ops.sal_weights(self.sal[1], self.value_scale) if self.sal else None   # the table's first use: ValueError outside the limits
        if nprob is True and not self.fss:
            raise ValueError("Validator: nprob=True takes the fss scales; give fss= as well, or the scales themselves")
        self.nprob = self.fss if nprob is True else ops.fss_scales(None if nprob is False else nprob)   # the scales, () for none; ValueError on a bad entry
        self.tracks = ops.tracks_spec(tracks)   # min_volume, or None; ValueError on a bad entry
        self.intensity_scale = bool(intensity_scale)
        self.ensemble = ops.ensemble_spec(ensemble, None)   # the member codes, True (resolved with the epoch's frames) or None; ValueError on a bad entry
        if self.ensemble and not 1.0 <= float(np.float32(self.value_scale)) < 256.0:
            raise ValueError(f"Validator: ensemble= keeps the members' levels as bytes, which needs value_scale finite with 1 <= floor(value_scale) <= 255, "
                             f"got {self.value_scale}")
        self._parts, _ = self._table(None)   # the spectrum and intensity-scale parts come with the block: their sizes follow the epoch's frames
        for part in self._parts:
            if len(part.pools) > ops.MAX_POOLS:   # a baseline's pass; pool_pairs has bounded the forecast's
                raise ValueError(f"Validator: the {part.name.split('/')[0]} baseline is scored at (1, 1) and at every pool, which makes {len(self.pools) + 1} pools; "
                                 f"a pass takes {ops.MAX_POOLS} (give (1, 1) among the pools, or one pool fewer)")
        self._thr = (ctypes.c_float * len(self.thresholds))(*self.thresholds)
        self._fwd = GraphedForward(model, client=self, keep_quant=True)
        self._block = self._last = None    # the epoch's accumulator block and the last batch's fp32 loss: they outlive the graphs
        self._frame = None                  # (H, W) of the epoch
        self._spectrum_frame = None         # (H, W) the block's spectrum table was sized for
        self._block_members = None          # M the block's ensemble table was sized for

    # ---- device state
    def _table(self, frame):
        """block_rows for this Validator's options; frame: (H, W) of the epoch, which sizes the spectrum and the intensity-scale parts (None:
        without those parts) and, with ensemble=True, says how many members there are (None: without that part)"""
        codes = self._codes(frame)
        return block_rows(self.seq_len, len(self.thresholds), self.pools, self.persistence, self.fss, bool(self.advection),
                          frame if self.spectrum else None, self._levels, sal=self.sal, nprob=self.nprob, tracks=self.tracks, objects=self.objects,
                          iscale=frame if self.intensity_scale else None, ensemble=len(codes) if codes else None)

    def _codes(self, frame):
        """the member codes for frames of (H, W): a tuple, or None (no ensemble, or ensemble=True before the frames are known).  ValueError for
        a transposing code on frames that are not square."""
        codes = ops.ensemble_spec(self.ensemble, None if frame is None else frame[0] == frame[1])
        return None if codes is True else codes

    def _block_for(self, device):
        """ONE allocation, the parts of block_parts; done() reduces it with one all-reduce"""
        if self._block is None:
            self._parts, total = self._table(self._frame)
            assert lib.query("adnm_valid_block_bytes", self.seq_len, len(self.thresholds)) == 8 * self._parts[0].size
            self._block = torch.zeros(total, dtype=torch.float64, device=device)
            self._last = torch.zeros((), dtype=torch.float32, device=device)
            self._spectrum_frame = self._frame
            self._block_members = len(self._codes(self._frame) or ())
        elif self._block.device != device:
            raise RuntimeError(f"Validator: one device per Validator (the block is on {self._block.device}, the batch on {device})")
        elif self.spectrum and self._spectrum_frame != self._frame:
            raise RuntimeError(f"Validator: spectrum=True keeps one frame size per Validator (the table in the block is for frames of "
                               f"{self._spectrum_frame[0]} x {self._spectrum_frame[1]}, the batch has {self._frame[0]} x {self._frame[1]})")
        elif self.intensity_scale and self._spectrum_frame != self._frame:
            raise RuntimeError(f"Validator: intensity_scale=True keeps one frame size per Validator (the tables in the block are for frames of "
                               f"{self._spectrum_frame[0]} x {self._spectrum_frame[1]}, the batch has {self._frame[0]} x {self._frame[1]})")
        elif self.ensemble and self._block_members != len(self._codes(self._frame)):
            raise RuntimeError(f"Validator: ensemble= keeps one number of members per Validator (the table in the block is for {self._block_members}, "
                               f"frames of {self._frame[0]} x {self._frame[1]} give {len(self._codes(self._frame))})")
        return self._block

    def _launch(self, ent, sx, pred, block, loss_out):
        B, T, H, W = ent["shape"]
        nthr, stream = len(self.thresholds), torch.cuda.current_stream().cuda_stream
        lib.call("adnm_valid_accum", pred.data_ptr(), ent["tgt"].data_ptr(), block.data_ptr(), loss_out.data_ptr(), self._thr, nthr, self.value_scale,
                 ent["loss"][0], ent["loss"][1], ent["loss"][2], ent["ws"].data_ptr(), ent["ws"].numel(), B * T, T, H * W, stream)
        if ent["ws_ssim"] is not None:
            lib.call("adnm_valid_ssim_accum", pred.data_ptr(), ent["tgt"].data_ptr(), block.data_ptr(), nthr, self.value_scale, ent["ws_ssim"].data_ptr(),
                     ent["ws_ssim"].numel(), B * T, T, H, W, stream)

        def source(field):
            """-> (pointer, sample stride, frame stride) of a scored field"""
            if field == "last":    # persistence: the last input frame of the sample, for every frame index
                t_in = sx.shape[1]
                return sx.data_ptr() + 4 * (t_in - 1) * H * W, t_in * H * W, 0
            return (pred if field == "pred" else ent["adv"]).data_ptr(), T * H * W, H * W   # contiguous (B, T, H, W)
        moved = False
        for part in self._parts[1:]:   # one launch per table, in the block's order
            table = block.data_ptr() + 8 * part.offset
            if part.field == "adv" and not moved:   # the advected field, in front of the first pass that scores it
                block_px, radius, echo = self.advection
                t_in, moved = sx.shape[1], True
                estimate, move, vectors = ("adnm_trec_flow", "adnm_advect_flow", ent["flow"]) if self.advection_flow else ("adnm_trec_motion", "adnm_advect", ent["motion"])
                lib.call(estimate, sx.data_ptr() + 4 * (t_in - 2) * H * W, sx.data_ptr() + 4 * (t_in - 1) * H * W, t_in * H * W, vectors.data_ptr(),
                         None, self.value_scale, block_px, radius, echo, ent["ws_trec"].data_ptr(), ent["ws_trec"].numel(), B, H, W, stream)
                lib.call(move, sx.data_ptr() + 4 * (t_in - 1) * H * W, t_in * H * W, vectors.data_ptr(), ent["adv"].data_ptr(), block_px, B, T, H, W, stream)
            src = source(part.field)
            if part.kind == "pool":
                lib.call("adnm_valid_pool_accum", *src, ent["tgt"].data_ptr(), table, self._thr, nthr, self.value_scale, ops.pool_table(part.pools), len(part.pools),
                         ent["ws_pool"].data_ptr(), ent["ws_pool"].numel(), B * T, T, H, W, stream)
            elif part.kind == "fss":
                lib.call("adnm_valid_fss_accum", *src, ent["tgt"].data_ptr(), table, self._thr, nthr, self.value_scale, ops.fss_table(self.fss), len(self.fss),
                         ent["ws_fss"].data_ptr(), ent["ws_fss"].numel(), B * T, T, H, W, stream)
            elif part.kind == "spectrum":
                lib.call("adnm_valid_spectrum_accum", *src, ent["tgt"].data_ptr(), table, self.value_scale, ent["ws_spectrum"].data_ptr(), ent["ws_spectrum"].numel(),
                         B * T, T, H, W, stream)
            elif part.kind == "joint":
                ws = ent["ws_joint"]
                lib.call("adnm_valid_joint_accum", *src, ent["tgt"].data_ptr(), table, self.value_scale, None if ws is None else ws.data_ptr(),
                         0 if ws is None else ws.numel(), B * T, T, H * W, stream)
            elif part.kind == "sal":
                lib.call("adnm_valid_sal_accum", *src, ent["tgt"].data_ptr(), table, self._thr, nthr, self.value_scale, self.sal[0], self._weights,
                         ent["ws_sal"].data_ptr(), ent["ws_sal"].numel(), B * T, T, H, W, stream)
            elif part.kind == "nprob":   # (no workspace: the query in open() answered 0)
                lib.call("adnm_valid_nprob_accum", *src, ent["tgt"].data_ptr(), table, self._thr, nthr, self.value_scale, ops.fss_table(self.nprob),
                         len(self.nprob), None, 0, B * T, T, H, W, stream)
            elif part.kind == "iscale":
                lib.call("adnm_valid_iscale_accum", *src, ent["tgt"].data_ptr(), table, self._thr, nthr, self.value_scale, ent["ws_iscale"].data_ptr(),
                         ent["ws_iscale"].numel(), B * T, T, H, W, stream)
            elif part.kind == "ensemble":   # the M members against the target: `pred` is member 0 of the same buffer (no workspace: the query answered 0)
                mem = ent["members"]
                ops.ensemble_accum_into(mem, B * T * H * W, T * H * W, H * W, ent["tgt"], table, self._thr, nthr, self.value_scale, mem.shape[0], B * T, T, H * W)
            elif part.kind == "tracks":
                lib.call("adnm_valid_tracks_accum", *src, ent["tgt"].data_ptr(), table, self._thr, nthr, self.value_scale, self.tracks,
                         ent["ws_tracks"].data_ptr(), ent["ws_tracks"].numel(), B * T, T, H, W, stream)
            else:   # objects
                ws = ent["ws_objects"]
                lib.call("adnm_valid_objects_accum", *src, ent["tgt"].data_ptr(), table, self._thr, nthr, self.value_scale, self.objects,
                         None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), B * T, T, H, W, stream)

    # ---- ForwardClient: what GraphedForward calls with the entry of one input shape
    def open(self, ent, x):
        """what the graph of one input shape points into: the static target and the two workspaces; and one eager run of the two entry
        points on a scratch block (a kernel's first launch must not happen inside a capture)"""
        B, T, H, W = shape = (x.shape[0], self.seq_len) + self._frame
        dev, nthr = x.device, len(self.thresholds)

        def workspace(entry, calls, limits, floor=16):
            """query, raise with the limits, allocate: ONE workspace of the largest need among `calls` (the query's argument tuples), at least
            `floor` bytes; None where nothing is needed"""
            need = [int(lib.query(entry, *args)) for args in calls]
            if min(need) < 0:
                raise RuntimeError(f"Validator: {limits}")
            size = max(need + [floor])
            return torch.empty(size, dtype=torch.uint8, device=dev) if size else None
        ws = workspace("adnm_valid_accum_ws_bytes", [(B * T, T, H * W, nthr)],
                       f"a batch of {B * T} frames of {H} x {W} is outside adnm_valid_accum's limits (frames <= 65535, pixels per frame < 2^24)")
        ws_ssim = None
        if self.ssim and H > 10 and W > 10:   # 11 x 11 windows need a valid region; smaller frames: SSIM is None
            ws_ssim = torch.empty(max(int(lib.query("adnm_valid_ssim_accum_ws_bytes", B * T, T, H, W, nthr)), 16), dtype=torch.uint8, device=dev)
        ws_pool = ws_fss = adv = motion = flow = ws_trec = ws_spectrum = ws_joint = ws_objects = ws_sal = ws_tracks = ws_iscale = None
        passes = [p.pools for p in self._parts if p.kind == "pool"]
        if passes:   # the passes follow one another on one stream: one workspace
            ws_pool = workspace("adnm_valid_pool_accum_ws_bytes", [(B * T, T, H, W, nthr, ops.pool_table(pools), len(pools)) for pools in passes],
                                f"pools {self.pools} on {B * T} frames of {H} x {W} are outside adnm_valid_pool_accum's limits "
                                "(no window larger than the frame, H and W < 32768)", floor=0)
        if self.fss:   # likewise
            ws_fss = workspace("adnm_valid_fss_accum_ws_bytes", [(B * T, T, H, W, nthr, ops.fss_table(self.fss), len(self.fss))],
                               f"fss on {B * T} frames of {H} x {W} is outside adnm_valid_fss_accum's limits (H and W < 32768)")
        if self.persistence or self.advection:
            sx, what = ent["sx"], "persistence" if self.persistence else "advection"
            if (sx.dtype != torch.float32 or sx.dim() not in (4, 5) or (sx.dim() == 5 and sx.shape[2] != 1) or tuple(sx.shape[-2:]) != (H, W)
                    or sx.shape[1] < 1 or not sx.is_contiguous()):
                raise RuntimeError(f"Validator: {what} needs the model's input as contiguous fp32 (B, T_in, 1, H, W) or (B, T_in, H, W) with the "
                                   f"target's {H} x {W} frames, got {sx.dtype} {tuple(sx.shape)}")
        if self.advection:
            if ent["sx"].shape[1] < 2:
                raise RuntimeError(f"Validator: advection estimates the motion from the last two input frames, the input has {ent['sx'].shape[1]}")
            block_px, radius, _ = self.advection
            ws_trec = workspace("adnm_trec_ws_bytes", [(B, H, W, block_px, radius)],
                                f"advection on {B} samples of {H} x {W} is outside adnm_trec_motion's limits (samples <= 65535, H and W < 32768, H*W < 2^24)")
            adv = torch.zeros(shape, dtype=torch.float32, device=dev)
            vectors = torch.zeros((B, -(-H // block_px), -(-W // block_px), 2), dtype=torch.int32, device=dev)
            motion, flow = (None, vectors) if self.advection_flow else (vectors, None)   # (adnm_trec_flow_ws_bytes is adnm_trec_ws_bytes)
        if self.spectrum:
            ws_spectrum = workspace("adnm_valid_spectrum_accum_ws_bytes", [(B * T, T, H, W)],
                                    f"spectrum on {B * T} frames of {H} x {W} is outside adnm_valid_spectrum_accum's limits (frames <= 65535, "
                                    f"{ops.SPECTRUM_LIMITS})", floor=0)
        if self.joint:
            ws_joint = workspace("adnm_valid_joint_accum_ws_bytes", [(B * T, T, H * W, self.value_scale)],
                                 f"joint on {B * T} frames of {H} x {W} is outside adnm_valid_joint_accum's limits (frames <= 65535, "
                                 f"H*W < 2^24, {ops.JOINT_LIMITS})", floor=0)
        if self.objects:
            ws_objects = workspace("adnm_valid_objects_accum_ws_bytes", [(B * T, T, H, W, nthr)],
                                   f"objects on {B * T} frames of {H} x {W} are outside adnm_valid_objects_accum's limits (frames <= 65535, "
                                   f"{ops.OBJECTS_LIMITS})", floor=0)
        if self.sal:
            ws_sal = workspace("adnm_valid_sal_accum_ws_bytes", [(B * T, T, H, W, nthr)],
                               f"sal on {B * T} frames of {H} x {W} is outside adnm_valid_sal_accum's limits (frames <= 65535, {ops.SAL_LIMITS})")
        if self.nprob and int(lib.query("adnm_valid_nprob_accum_ws_bytes", B * T, T, H, W, nthr, ops.fss_table(self.nprob), len(self.nprob))) != 0:
            raise RuntimeError(f"Validator: nprob on {B * T} frames of {H} x {W} is outside adnm_valid_nprob_accum's limits (frames <= 65535, H and W < 32768, "
                               "H*W < 2^24)")
        if self.intensity_scale:   # the passes follow one another on one stream: one workspace
            ws_iscale = workspace("adnm_valid_iscale_accum_ws_bytes", [(B * T, T, H, W, nthr)],
                                  f"intensity_scale on {B * T} frames of {H} x {W} is outside adnm_valid_iscale_accum's limits (frames <= 65535, "
                                  f"H and W <= {ops.MAX_ISCALE_SIDE})")
        if self.tracks:
            ws_tracks = workspace("adnm_valid_tracks_accum_ws_bytes", [(B * T, T, H, W, nthr)],
                                  f"tracks on {B * T} frames in volumes of {T} x {H} x {W} are outside adnm_valid_tracks_accum's limits (frames <= 65535, "
                                  f"{ops.TRACK_LIMITS})")
        codes = self._codes(self._frame)
        if codes:
            M = len(codes)
            if x.dtype != torch.float32 or x.dim() < 3 or tuple(x.shape[-2:]) != (H, W) or not x.is_contiguous():
                raise RuntimeError(f"Validator: ensemble= transforms the model's input, which must be contiguous fp32 (B, ..., H, W) with the target's "
                                   f"{H} x {W} frames, got {x.dtype} {tuple(x.shape)}")
            if int(lib.query("adnm_valid_ens_accum_ws_bytes", B * T, T, H * W, nthr, M, self.value_scale)) != 0 or x.numel() // (H * W) > 65535:
                raise RuntimeError(f"Validator: an ensemble of {M} on {B * T} frames of {H} x {W} is outside adnm_valid_ens_accum's or adnm_d4_members' limits "
                                   f"({ops.ENSEMBLE_LIMITS}; input planes <= 65535)")
            ent.update(codes=(ctypes.c_int * M)(*codes), xin=torch.zeros((M * B,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev),
                       members=torch.zeros((M,) + shape, dtype=torch.float32, device=dev))
            # the two directions once, eagerly, on the buffers and so on the access paths the graph will use
            ops.d4_members_into(ent["sx"], ent["xin"], ent["codes"], M, False)
            ops.d4_members_into(torch.zeros_like(ent["members"]), ent["members"], ent["codes"], M, True)
        else:
            ent.update(codes=None, xin=None, members=None)
        ent.update(shape=shape, tgt=torch.zeros(shape, dtype=torch.float32, device=dev), ws=ws, ws_ssim=ws_ssim, ws_pool=ws_pool, ws_fss=ws_fss,
                   ws_spectrum=ws_spectrum, ws_joint=ws_joint, ws_objects=ws_objects, ws_sal=ws_sal, ws_tracks=ws_tracks, ws_iscale=ws_iscale, adv=adv, motion=motion, flow=flow, ws_trec=ws_trec,
                   loss=(float(self.loss_fn.omega_t), float(self.loss_fn.alpha), float(self.loss_fn.gamma)))
        scratch = torch.zeros_like(self._block_for(dev))
        self._launch(ent, ent["sx"], ent["tgt"], scratch, torch.zeros((), dtype=torch.float32, device=dev))

    def model_input(self, ent, sx):
        """ensemble: the M transformed copies of the static input, member-major: sample m * B + b of the forward is member m of sample b"""
        if ent["xin"] is None:
            return sx
        ops.d4_members_into(sx, ent["xin"], ent["codes"], ent["members"].shape[0], False)
        return ent["xin"]

    def check(self, ent, out):
        B, T, H, W = ent["shape"]
        if ent["members"] is not None:
            B *= ent["members"].shape[0]
        if out.dtype != torch.float32 or out.numel() != B * T * H * W or tuple(out.shape[:2]) != (B, T):
            raise RuntimeError(f"Validator: the model's output {tuple(out.shape)} {out.dtype} does not match the target's (B, T, H, W) = {(B, T, H, W)} fp32")

    def after(self, ent, sx, out):
        if ent["members"] is None:
            ent["pred"] = ent["control"] = out.contiguous()   # (the model emits it contiguous; a copy made here belongs to the graph's pool and is kept with it)
        else:   # the symmetries undone; every pass but the ensemble's scores member 0, the contiguous control forecast
            mem = ent["members"]
            ops.d4_members_into(out.contiguous(), mem, ent["codes"], mem.shape[0], True)
            ent["pred"] = mem[0]
            ent["control"] = mem[0].view((mem.shape[1],) + tuple(out.shape[1:]))   # in the model's own shape
        self._launch(ent, sx, ent["pred"], self._block, self._last)

    # ---- the public surface
    def step(self, x, tgt):
        """x: the model's input; tgt: (B, seq_len, H, W) or (B, seq_len, 1, H, W) fp32, both on the GPU.  Adds the batch to the epoch's
        block.  -> the model's output (the graph's static tensor: valid until the next step of this shape)."""
        if not (torch.is_tensor(x) and x.is_cuda and torch.is_tensor(tgt) and tgt.is_cuda):
            raise RuntimeError("Validator runs on GPU tensors only (there is no CPU path here)")
        if tgt.dtype != torch.float32 or tgt.dim() not in (4, 5) or (tgt.dim() == 5 and tgt.shape[2] != 1):
            raise RuntimeError(f"Validator: the target must be fp32 (B, T, H, W) or (B, T, 1, H, W), got {tgt.dtype} {tuple(tgt.shape)}")
        if tgt.shape[1] != self.seq_len:
            raise RuntimeError(f"Validator: the target has {tgt.shape[1]} frames per sample, seq_len is {self.seq_len}")
        if tgt.shape[0] != x.shape[0] or tgt.device != x.device:
            raise RuntimeError(f"Validator: input {tuple(x.shape)} on {x.device} and target {tuple(tgt.shape)} on {tgt.device} do not belong together")
        shape = (tgt.shape[0], tgt.shape[1], tgt.shape[-2], tgt.shape[-1])
        self._begin(shape, x.device)
        ent = self._fwd.entry(x)
        if ent["shape"] != shape:
            raise RuntimeError(f"Validator: input {tuple(x.shape)} came with a target of {ent['shape']} before, now {shape}")
        ent["tgt"].view(tgt.shape).copy_(tgt, non_blocking=True)
        return self._result(self._fwd.replay(ent, x))

    def _result(self, ent):
        """what a step returns: the model's output, or with ensemble= the control forecast (member 0) in the model's output shape"""
        return ent["out"] if ent["members"] is None else ent["control"]

    def _begin(self, shape, device):
        """a batch of (B, T, H, W) targets enters the epoch: its frames are the epoch's, the block is on its device"""
        if self._frame is None:
            self._frame = shape[2:]
        elif self._frame != shape[2:]:
            raise RuntimeError(f"Validator: frames of {shape[2]} x {shape[3]} in an epoch of {self._frame[0]} x {self._frame[1]} frames (done(reset=True) first)")
        self._block_for(device)

    def step_from(self, feed):
        """step() on the next batch of a dataio.ResidentDataset.  Once the feed's shape has a captured graph, the batch is fetched
        straight into that graph's static input and target (one launch; no copy of either, and none of a buffer onto itself); before
        that (the first batch of a shape) into tensors of its own, which step() copies while it captures."""
        B, T, _, H, W = feed.tgt_shape
        if T != self.seq_len:
            raise RuntimeError(f"Validator: the feed has {T} target frames per sample, seq_len is {self.seq_len}")
        ent = self._fwd._graphs.get((tuple(feed.x_shape), torch.float32, feed.device))
        if ent is None or ent["graph"] is None:
            return self.step(*feed.fetch())
        if ent["shape"] != (B, T, H, W):
            raise RuntimeError(f"Validator: input {feed.x_shape} came with a target of {ent['shape']} before, the feed gives {(B, T, H, W)}")
        self._begin((B, T, H, W), feed.device)
        feed.fetch_into(ent["sx"], ent["tgt"])
        return self._result(self._fwd.replay(ent, ent["sx"]))

    def members(self, x):
        """ensemble: the member forecasts of the last batch of x's shape, symmetries undone: the graph's static fp32 (M, B, T, H, W) tensor,
        member 0 the control, valid until the next step of that shape (ops.ensemble_product forms the mean and the exceedance probabilities)"""
        ent = self._fwd._graphs.get((tuple(x.shape), x.dtype, x.device))
        if not self.ensemble or ent is None or ent.get("members") is None:
            raise RuntimeError("Validator.members: needs ensemble= and a step() on an input of this shape, dtype and device first")
        return ent["members"]

    def advected(self, x):
        """the advected forecast of the last batch of x's shape: the graph's static fp32 (B, T, H, W) tensor, valid until the next step
        of that shape (Forecaster.render can colour it)"""
        ent = self._fwd._graphs.get((tuple(x.shape), x.dtype, x.device))
        if not self.advection or ent is None or ent.get("adv") is None:
            raise RuntimeError("Validator.advected: needs advection= and a step() on an input of this shape, dtype and device first")
        return ent["adv"]

    def flow(self, x):
        """advection_flow: the block flow of the last batch of x's shape: the graph's static int32 (B, nby, nbx, 2) tensor, (uy, ux) in 1/16 px
        per frame, valid until the next step of that shape (ops.flow_field spreads it to the dense field)"""
        ent = self._fwd._graphs.get((tuple(x.shape), x.dtype, x.device))
        if not self.advection_flow or ent is None or ent.get("flow") is None:
            raise RuntimeError("Validator.flow: needs advection_flow=True and a step() on an input of this shape, dtype and device first")
        return ent["flow"]

    @property
    def last_loss(self):
        """the fp32 loss of the last batch: a 0-dim device tensor (reading it synchronises; the epoch's sum is in done())"""
        return self._last

    def done(self, reset=False, per_lead=False):
        """-> what GpuEvaluator.done() returns (the same keys, the same aggregation; SSIM None when ssim=False or the frames are too small
        for the window) plus "loss_sum" (what train.py:163 / :201 accumulate and compare against `best`), "loss_mean" (over the finite
        batches), "batches", "samples", "nonfinite".  With a process_group the blocks of all ranks are summed first.  The one host read.
        pools: plus "pooled": {(size, stride): {"threshold_metrics", "FAR"}}, the same scores counted per max-pool window.
        persistence: plus "persistence": {"threshold_metrics", "FAR", "pooled": {...}}, the last input frame held for every frame index,
        scored on the same batches.  per_lead=True: plus "per_lead": length-T arrays "RMSE", "MAE", "SSIM" (or None) and
        "threshold_metrics"[thr][TP | FN | FP | TN | CSI | POD | FAR | HSS], and the same under "pooled" / "persistence" where those exist.
        fss: plus "fss": {n: {thr: FSS}} (NaN where neither field has an event), "fss_useful": {thr: 0.5 + f_o / 2}, and "fss" under
        "persistence" and, as length-T arrays, under "per_lead" and "per_lead"/"persistence" where those exist.
        advection: plus "advection" and "per_lead"/"advection", built like "persistence": the last input frame moved along its
        block-matched motion, scored on the same batches.  advection_flow: the same entries from the frame carried along the sub-pixel flow
        (DESIGN.md §4p), and "advection"/"scheme" = "flow".
        spectrum: plus "spectrum" {"wavenumber", "wavelength_px", "target", "forecast", "ratio", "coherence", "effective_resolution_px"}
        (aggregate) and, as (T, R) arrays with a length-T "effective_resolution_px", "per_lead"/"spectrum".
        joint: plus "joint" {"levels", "histogram", "marginal_target", "marginal_forecast", "curves", "conditional_mean", "qq", "correlation",
        "mean_error"} (joint_entries of the table summed over the horizon) and "per_lead"/"joint", the same with a leading T axis.
        objects: plus "objects" {"min_area", thr: {"target", "forecast", "count_bias", "size_bias", "object_POD", "object_FAR", "object_CSI",
        "size_bin_edges"}} (object_entries of the table summed over the horizon) and "per_lead"/"objects", the same with a leading T axis.
        sal: plus "sal" {"min_area", "intensity", thr: {"A", "abs_A", "S", "abs_S", "L1", "L2", "L", "frames_A", "frames_L1", "frames_S",
        "missed_frames", "false_frames"}} (sal_entries of the table summed over the horizon) and "per_lead"/"sal", the same with a leading T axis.
        nprob: plus "nprob" {n: {thr: {"histogram", "base_rate", "brier", "reliability", "resolution", "uncertainty", "brier_skill", "roc",
        "roc_area", "reliability_diagram"}}} (nprob_entries of the table summed over the horizon) and "per_lead"/"nprob", the same with a leading T axis.
        tracks: plus "tracks" {"min_volume", thr: {"target", "forecast", "count_bias", "duration_bias", "survival_bias", "track_POD", "track_FAR",
        "track_CSI"}} (track_entries of the table).  Its births, deaths, alive and survival arrays are per lead time already, so per_lead=True
        adds nothing for tracks.
        intensity_scale: plus "intensity_scale" {"scale_px", "domain_px", "levels", thr: {"mse", "skill", "mse_share", "mse_total", "mse_random",
        "base_rate", "bias", "energy_target", "energy_forecast", "energy_rel_diff"}} (intensity_scale_entries of the table summed over the
        horizon), the same under "persistence" and "advection" where those exist, and under "per_lead" with a leading T axis.
        ensemble: plus "ensemble" {"members", "pixels", "dry", "crps", "crps_fair", "mae_control", "crpss", "spread", "rmse_mean", "spread_skill",
        "rank_histogram", "rank_histogram_wet", thr: {what nprob reports, for p = c / M}} (ensemble_entries of the table summed over the horizon; levels
        in units of the quantised value) and "per_lead"/"ensemble", the same with a leading T axis.  Every other entry is the control's."""
        if self._block is None or self._frame is None:
            raise RuntimeError("Validator.done: no batch since the last reset")
        blk = reduce_block(self._block.clone(), self.process_group) if self.process_group is not None else self._block
        host = blk.cpu().numpy()   # the one device -> host read
        H, W = self._frame
        area = (H - 10) * (W - 10) if (self.ssim and H > 10 and W > 10) else None
        res = aggregate(host, self.thresholds, self.seq_len, H * W, area, pools=self.pools, persistence=self.persistence, per_lead=per_lead,
                        fss=self.fss, advection=bool(self.advection), spectrum=self._frame if self.spectrum else None, joint=self._levels, objects=self.objects,
                        sal=dict(min_area=self.sal[0], intensity=self.sal[1]) if self.sal else None, nprob=self.nprob, tracks=self.tracks,
                        intensity_scale=self._frame if self.intensity_scale else None, ensemble=self._block_members or None)
        if self.advection_flow:
            res["advection"]["scheme"] = "flow"
        if reset:
            self.reset()
        return res

    def reset(self):
        if self._block is not None:
            self._block.zero_()
        self._frame = None

    def close(self):
        """Give the captured graphs and what they point into back (GraphedForward.close); the block and its sums stay.  Idempotent."""
        self._fwd.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
