"""The evaluation side of the hot path, on the GPU: the reference's validate.py:92-125 runs
model.eval() under no_grad, copies every prediction to numpy and walks SimplifiedEvaluator's Python loops
(datasets/Shanghai_metrics.py:49-152) frame by frame.  Here

  * GraphedForward replays the forward as ONE captured hipGraph with no saved activations (no_grad), and
  * GpuEvaluator keeps the contingency counts and the squared / absolute error sums on the device (one HIP pass per batch,
    csrc/dataio.hip::eval_counts) and only reads a (frames, 18) table back in done().

GpuEvaluator mirrors SimplifiedEvaluator's surface: __init__(seq_len, value_scale, thresholds), evaluate(true_batch, pred_batch),
done() -> {"threshold_metrics": {thr: TP, TN, FP, FN, CSI, POD, HSS}, "FAR", "RMSE", "SSIM", "LPIPS"}, reset().  SSIM is the reference's
cal_ssim (Shanghai_metrics.py:132-152: 11x11 Gaussian windows, valid region, float64) as one HIP pass per batch (csrc/dataio.hip::eval_ssim),
pinned by the reference's own code run with the two cv2 calls replaced by their documented formulas (cv2 is not installed in the build
container).  LPIPS (a downloaded AlexNet) is outside the hot path and not reproduced: its entry is None."""
import ctypes

import numpy as np
import torch

from . import lib, ops


class ForwardClient:
    """What a GraphedForward hands its per-shape entry `ent` (a dict) to.  Every method here is a no-op or the identity; a client keeps
    whatever belongs to one input shape IN `ent`, which lives and dies with that shape's graph."""

    def open(self, ent, x):
        """Once per input shape, outside any capture: allocate what this shape's graph will point into, into `ent`, and launch eagerly
        once every kernel after() will launch (a kernel's first launch must not be captured)."""

    def model_input(self, ent, sx):
        """-> the model's input, made from the static input `sx`.  Runs in both warm-up forwards and inside the capture."""
        return sx

    def check(self, ent, out):
        """Once per input shape, on the second warm-up forward's output, BEFORE the capture begins: may raise, may allocate into `ent`."""

    def after(self, ent, sx, out):
        """Inside the capture only, behind the forward (out: the graph's static output)."""


class GraphedForward:
    """model.eval() forward under no_grad, captured once per input shape and replayed (validate.py:101-104).  The graph of a model whose
    parameters a FlatTrainer holds reads the trainer's narrow weight shadow (ops.ShadowSet) through baked-in pointers: every call first
    rewrites the shadows it captured against if a parameter was written since (a checkpoint load, an in-place op), and the graph keeps
    them alive, so it may outlive the trainer.  close() (or __del__) gives the graphs back.

    Per (shape, dtype, device) there is ONE entry: the graph, its static input "sx" and output "out", its split-K scope, shadows and
    fp8 pin, and whatever the client (ForwardClient) put there.  fwd(x) is fwd.replay(fwd.entry(x), x)["out"]; a client that fills static
    buffers of its own does so between the two.  An entry whose open, warm-up, check or capture raised is not kept.
    keep_quant: in fp8, while a record's flag is set the GEMMs of ANY forward collect max |activation| into the delayed-scaling table.
    An evaluation forward must not move the training run's next scales: the graph saves the table in front of the forward and puts it
    back behind it, and the first call of a shape (its eager warm-up forwards collect too) runs between a snapshot and its restore."""

    def __init__(self, model, client=None, keep_quant=False):
        self.model, self.client, self.keep_quant = model, ForwardClient() if client is None else client, keep_quant
        self._graphs = {}

    def entry(self, x):
        """-> the entry of x's (shape, dtype, device), made on first sight (the static input, the client's open()); not captured yet"""
        key = (tuple(x.shape), x.dtype, x.device)
        ent = self._graphs.get(key)
        if ent is None:
            fp8 = self.keep_quant and ops.mfma_precision() == "fp8"
            ent = {"key": key, "graph": None, "sx": x.detach().clone(), "pin": None, "qsave": torch.empty_like(ops.QUANT.table(x.device)) if fp8 else None}
            self.client.open(ent, x)
            self._graphs[key] = ent
        return ent

    def _body(self, ent):
        sx, qsave = ent["sx"], ent["qsave"]
        if qsave is not None:
            qsave.copy_(ops.QUANT.table(sx.device))
        out = self.model(self.client.model_input(ent, sx))
        if qsave is not None:
            ops.QUANT.table(sx.device).copy_(qsave)
        self.client.after(ent, sx, out)
        return out

    def _capture(self, ent):
        sx, was_training = ent["sx"], self.model.training
        try:
            ptrs = [p.data_ptr() for p in self.model.parameters()]
            ent["shadows"] = [s for s in ops.SHADOWS.sets(sx.device) if any(s.lo <= q < s.hi for q in ptrs)]
            for s in ent["shadows"]:   # (the capture cannot rewrite a stale one)
                s.ensure_current()
            self.model.eval()
            warm = [None]

            def forward():
                warm[0] = self.model(self.client.model_input(ent, sx))
            ops.warm_up(forward, 2)
            self.client.check(ent, warm.pop())
            g = torch.cuda.CUDAGraph()
            # the graph's split GEMM launches get their own uncached workspace (kept with the graph: a training graph replayed on
            # another stream beside this one must not share it); fp8: the quantisation table's rows stay put while the graph lives
            ent["scope"] = ops.SPLITWS.open_scope(sx.device)
            ent["pin"] = ops.QUANT.pinned(sx.device) if ops.mfma_precision() == "fp8" else None
            ent["out"] = ops.capture(g, lambda: self._body(ent), ent["scope"])
        except BaseException:
            self._graphs.pop(ent["key"], None)
            if ent["pin"] is not None:
                ent["pin"].release()
            raise
        finally:
            self.model.train(was_training)
        ent["graph"] = g

    @torch.no_grad()
    def replay(self, ent, x):
        """x into the entry's static input and one replay of its graph, captured first if there is none yet.  -> ent"""
        if ent["graph"] is None:
            snap = ops.QUANT.snapshot(x.device) if ent["qsave"] is not None else None
            try:
                self._capture(ent)
                return self.replay(ent, x)
            finally:
                if snap is not None:
                    ops.QUANT.restore(x.device, snap)
        for s in ent["shadows"]:
            s.ensure_current()
        if x is not ent["sx"]:   # (a client that filled the static input in place hands it back: no copy onto itself)
            ent["sx"].copy_(x, non_blocking=True)
        ent["graph"].replay()
        return ent

    def __call__(self, x):
        return self.replay(self.entry(x), x)["out"]

    def close(self):
        """Give the captured graphs back now: the graphs first, then what their launches point into (the entries: static tensors, the
        client's buffers, split-K workspaces, the weight shadows), then the pins on the fp8 quantisation table.  Idempotent; __del__
        calls it."""
        graphs, self._graphs = self._graphs, {}
        pins = [ent["pin"] for ent in graphs.values() if ent["pin"] is not None]
        for ent in graphs.values():
            ent["graph"] = None
        graphs = None
        for pin in pins:
            pin.release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def contingency_metrics(sums, thresholds):
    """sums: the TP, FN, FP, TN counts per threshold, summed over everything evaluated (4 * nthr integers in doubles) -> (the
    threshold_metrics dictionary, the FAR of every threshold), as SimplifiedEvaluator.done states them (Shanghai_metrics.py:218-290)."""
    metrics, all_far = {}, []
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, thr in enumerate(thresholds):
            TP, FN, FP, TN = sums[4 * k:4 * k + 4]
            csi, pod = TP / (TP + FP + FN), TP / (TP + FN)
            hss = (2 * (TP * TN - FP * FN)) / (FP ** 2 + FN ** 2 + 2 * TP * TN + (FP + FN) * (TP + TN))
            all_far.append(FP / (TP + FP))
            key = int(thr) if float(thr).is_integer() else thr
            metrics[key] = {"TP": TP, "TN": TN, "FP": FP, "FN": FN, "CSI": csi, "POD": pod, "HSS": hss}
    return metrics, all_far


class GpuEvaluator:
    def __init__(self, seq_len, value_scale, thresholds=(20, 30, 35, 40)):
        self.seq_len, self.value_scale, self.thresholds = seq_len, float(value_scale), [float(t) for t in thresholds]
        if not 1 <= len(self.thresholds) <= 8:
            raise ValueError("1..8 thresholds")
        self._thr = (ctypes.c_float * len(self.thresholds))(*self.thresholds)
        self.reset()

    def reset(self):
        self._tables = []   # one (B, T, 4*nthr+2) device tensor per evaluate() call
        self._ssim = []     # one (B, T) device tensor of SSIM-map sums per evaluate() call (None for frames too small for the window)
        self.total = 0

    def evaluate(self, true_batch, pred_batch):
        """true_batch / pred_batch: (B, T, H, W) or (B, T, 1, H, W) fp32 GPU tensors in [0, 1] (clipped here as the reference does)."""
        t, p = true_batch, pred_batch
        if not (torch.is_tensor(t) and t.is_cuda and torch.is_tensor(p) and p.is_cuda):
            raise RuntimeError("GpuEvaluator runs on GPU tensors only (there is no numpy path here)")
        if t.dim() == 5:
            t, p = t.squeeze(2), p.squeeze(2)
        t, p = t.float().contiguous(), p.float().contiguous()
        B, T, H, W = t.shape
        nthr = len(self.thresholds)
        out = torch.empty((B, T, 4 * nthr + 2), dtype=torch.float32, device=t.device)
        nb = lib.query("adnm_eval_counts_ws_bytes", B * T, H * W, nthr)
        ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=t.device)
        lib.call("adnm_eval_counts", t.data_ptr(), p.data_ptr(), out.data_ptr(), self._thr, nthr, self.value_scale, ws.data_ptr(), nb, B * T, H * W,
                 torch.cuda.current_stream().cuda_stream)
        ssim = None
        if H > 10 and W > 10:   # 11 x 11 windows need a valid region
            ssim = torch.empty((B, T), dtype=torch.float32, device=t.device)
            nb2 = lib.query("adnm_eval_ssim_ws_bytes", B * T, H, W)
            ws2 = torch.empty(max(int(nb2), 16), dtype=torch.uint8, device=t.device)
            lib.call("adnm_eval_ssim", t.data_ptr(), p.data_ptr(), ssim.data_ptr(), self.value_scale, ws2.data_ptr(), nb2, B * T, H, W,
                     torch.cuda.current_stream().cuda_stream)
        self._tables.append((out, H * W))
        self._ssim.append((ssim, (H - 10) * (W - 10)))
        self.total += B

    def done(self):
        """Same aggregation as SimplifiedEvaluator.done (Shanghai_metrics.py:218-290)."""
        nthr = len(self.thresholds)
        tabs = [(t.double().cpu().numpy(), hw) for t, hw in self._tables]   # the one device -> host read
        counts = np.concatenate([t[..., :4 * nthr] for t, _ in tabs], axis=0)   # (samples, T, 4*nthr)
        mse = np.concatenate([t[..., 4 * nthr + 1] / hw for t, hw in tabs], axis=0)   # (samples, T)
        mae = np.concatenate([t[..., 4 * nthr] / hw for t, hw in tabs], axis=0)
        metrics, all_far = contingency_metrics(counts.sum(axis=(0, 1)), self.thresholds)
        rmse = float(np.mean(np.sqrt(np.mean(mse, axis=0))))
        return {"threshold_metrics": metrics, "FAR": float(np.mean(all_far)), "RMSE": rmse, "MAE": float(mae.mean()), "MSE": float(mse.mean()),
                "SSIM": (float(np.mean(np.concatenate([s.double().cpu().numpy() / area for s, area in self._ssim], axis=0)))
                         if self._ssim and all(s is not None for s, _ in self._ssim) else None),
                "LPIPS": None}
