"""The training step around the hot path, MI355X-style:

    [hipGraph 0]   forward -> loss -> backward of the LAST stage (refiner)       -> its gradients land in flat_g[bucket 0]
    [RCCL]         all-reduce of bucket 0 on RCCL's stream over xGMI ............  runs beside:
    [hipGraph 1]   backward of the stage before it (decoder blocks)             -> flat_g[bucket 1]
    [RCCL]         all-reduce of bucket 1 ........................................  beside graph 2 (e2ds + fusion), and so on down to the
    [hipGraph K-1] backward of the FIRST stage (encoder1-3)                     -> the last, smallest bucket: the only exposed all-reduce
    [3 HIP launches]   global grad-norm, clip_grad_norm_ scaling, AdamW on flat p / g / m / v

replacing the reference's nn.DataParallel scatter/replicate/gather (train.py:99-102), its per-tensor
clip_grad_norm_ (train.py:140) and torch.optim.AdamW over 669 tensors (train_untils.py:35-42).  On one GPU (or with
overlap=False) there is ONE graph and one bucket.  The stage cuts come from the model (forward_stages(): SURVEY.md §8e's order
refiner -> decoder -> e2ds / fusion -> encoder4-6 -> encoder1-3; or the older two-stage forward_stage1 / forward_stage2).

  * Parameters that receive gradients are re-homed as views into one flat buffer (state_dict unchanged), so the
    optimiser is a single streaming kernel and the gradient collective is a few LARGE messages in reverse execution order
    (refiner -> decoder -> encoder) — the right shape for xGMI rings.  The 307 parameters the reference never
    gives a gradient (e2ds[3..6], att1..4, ...) are discovered by a dry-run backward and left out: they are never decayed nor
    updated, exactly like torch.optim.AdamW skipping p.grad is None.
  * fwd+bwd is captured once as hipGraphs (our kernels are enqueued through ctypes on torch's capture stream; all memory
    comes from torch's graph-private pool) and replayed.  The collectives and the optimiser stay outside the graphs, so
    learning-rate schedules and the adaptive clip threshold of train.py:122-130 remain ordinary host-side floats, and the
    collectives are plain torch.distributed calls between graph launches (nothing RCCL-specific is captured).
  * reduce_dtype="bf16": the wire format of the collective is bf16 (146 MB instead of 292 MB); sums are formed by RCCL in
    bf16, the 1/world average and the return to fp32 happen in one HIP pass.
"""
import contextlib
import gc
import weakref

import torch
import torch.distributed as dist

from . import lib, ops


class FlatTrainer:
    def __init__(self, model, loss_fn, lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.0,
                 process_group=None, use_graph=True, fused=True, overlap="auto", reduce_dtype="f32", stages=None, defer_folds=True, side_stream=False,
                 nstages=None, accum_steps=1, monitor=False, ema_decay=None, ema_warmup=True):
        """overlap: cut the backward at the model's stage boundaries and all-reduce every stage's gradients while the backward of the
        stages before it runs.  "auto" = whenever there is more than one rank.  `stages` is the older name of the same switch
        (True / False).  nstages: None = every stage the model offers (forward_stages(): 5 for ADNM-UNet); 2 = the two-stage cut
        (encoder | decoder + refiner).
        accum_steps: k calls of step() make ONE optimiser step on the mean gradient of their k micro-batches (train.py:136-145 with
        loss.backward() repeated before optimizer.step()); see step().
        monitor: keep the epoch's statistics (train.py:140-153: gradient norms, clip count, summed loss) in device memory — stats()
        reads them with ONE synchronising copy per epoch instead of two .item() per step — and SKIP every optimiser step whose
        gradient is not finite (parameters, moments, step counter, shadow and fp8 table stay as they were).  False: nothing of this
        exists, the step is launch for launch what it was.
        ema_decay: a float in [0, 1] keeps an exponential moving average of the parameters in a second flat fp32 buffer (self.ema, 4 bytes
        per parameter: ~0.29 GB for ADNM-UNet), moved by one HIP pass behind every APPLIED optimiser step (once per accumulation cycle; a
        skipped step leaves it alone): ema = d * ema + (1 - d) * p with d = ema_decay, or, ema_warmup=True, min(ema_decay, (1 + t) /
        (10 + t)) at optimiser step t, so that a young average is not dominated by the initial weights.  ema_weights() makes the model
        compute with it, ema_info() reads the decay in use and the number of updates.  None: nothing of this exists."""
        self.model, self.loss_fn = model, loss_fn
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_norm
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.use_graph, self.fused = use_graph, fused
        if stages is not None:
            overlap = bool(stages) if stages != "auto" else "auto"
        two = hasattr(model, "forward_stage1") and hasattr(model, "forward_stage2") and hasattr(model, "stage1_parameters")
        multi = hasattr(model, "forward_stages")
        self.staged = (two or multi) and (self.world > 1 if overlap == "auto" else bool(overlap))
        self.stage_defs = None   # [(function, set of parameter ids)] in forward order
        if self.staged:
            if multi and nstages != 2:
                defs = [(fn, {id(p) for m in mods for p in m.parameters()}) for fn, mods in model.forward_stages()]
                if nstages is not None and nstages < len(defs):   # merge the FIRST stages (the last buckets) down to nstages
                    k = len(defs) - nstages + 1
                    fns, ids = [f for f, _ in defs[:k]], set().union(*[i for _, i in defs[:k]])

                    def merged(*a, _fns=fns):
                        for f in _fns:
                            a = f(*a)
                        return a
                    defs = [(merged, ids)] + defs[k:]
                self.stage_defs = defs
            else:
                first = {id(p) for p in model.stage1_parameters()}
                self.stage_defs = [(model.forward_stage1, first), (model.forward_stage2, None)]   # None: every other parameter
        assert reduce_dtype in ("f32", "bf16")
        self.reduce_dtype = reduce_dtype
        self.defer_folds = defer_folds
        if side_stream:   # the keyword survives for callers that pass False; the lane it switched on measured slower and was removed
            raise ValueError("FlatTrainer(side_stream=True): the side-stream lane for weight gradients was removed (it measured slower, "
                             "see DESIGN.md); pass side_stream=False or leave the argument out")
        self._steps = 0
        # gradient accumulation: micro-steps per optimiser step, micro-steps done in the running cycle, the fp32 sum (only when k > 1)
        self._accum_steps = self._check_accum(accum_steps)
        self._micro = 0
        self.acc = None
        # the flat layout (_flatten)
        self.used = None
        self.flat_p = self.flat_g = self.exp_avg = self.exp_avg_sq = self.state = self.comm = self.ws = None
        self.groups, self.late, self.early, self.g_views, self.offs, self.gathered = [], [], [], [], [], []
        self.buckets, self.group_ranges = [], []
        self.n = self.n_late = 0
        # the narrow shadow (_setup_shadows; bf16 / fp8 configurations)
        self.fp8 = False
        self.shadow, self.shadow_mode, self._shadow = None, 0, None   # _shadow: its ops.ShadowSet
        self.seg_end = self.seg_rec = None
        # what the captures own (_prepare); _release_captures() is the one place that gives it back
        self.graph = self.graph2 = self.tail = None
        self.graphs = []
        self.static_loss = self._carry = self._cuts = self.sx = self.st = self._feed = None
        self.hyper = self._hyper_host = None   # [lr, max_norm] as the tail graph reads them, and the host's copy
        self._splitws = None                   # the split-K capture scope of all graphs (ops.SPLITWS)
        self._pin = None                       # the pin on the fp8 table (ops.QUANT.pinned)
        # monitor=True: the statistics block (include/adnm_hip.h: adnm_step_guard), allocated with the flat buffers; the tail graph holds
        # its address.  fused=False keeps the same nine doubles and takes the decision on the host (_skip_host)
        self.monitor = bool(monitor)
        self._stats = None
        self._skip_host = False
        self._norm_host = None
        # a state loaded before the flat buffers exist (load_state_dict): applied as the last act of _flatten; its fp8 part after the
        # calibration of prepare() has made the table's rows
        self._pending = self._pending_quant = None
        self._pending_ema = True
        # ema_decay is not None: the average (laid out like flat_p, allocated with it), [the d of the last update, updates applied] as
        # adnm_ema_update keeps them, and whether ema_weights() is open (flat_p and ema then hold each other's values)
        self.ema_decay, self.ema_warmup = self._check_ema_decay(ema_decay), bool(ema_warmup)
        self.ema = self._ema_info = None
        self._ema_open = False

    # ------------------------------------------------------------------ gradient accumulation
    @staticmethod
    def _check_accum(k):
        if isinstance(k, bool) or int(k) != k or int(k) < 1:
            raise ValueError(f"FlatTrainer: accum_steps={k!r} must be an integer >= 1")
        return int(k)

    @property
    def accum_steps(self):
        return self._accum_steps

    @accum_steps.setter
    def accum_steps(self, k):
        k = self._check_accum(k)
        if self._micro != 0:
            raise RuntimeError(f"FlatTrainer: accum_steps assigned in mid-cycle (micro-step {self._micro} of {self._accum_steps}): the "
                               "accumulator holds a partial sum; finish the cycle first")
        self._accum_steps = k
        if k == 1:
            self.acc = None

    @property
    def micro_step(self):
        """micro-steps done in the running cycle: 0 (between cycles) .. accum_steps - 1 (the next step() is the optimiser step)"""
        return self._micro

    def _accumulator(self):
        """the fp32 sum of the cycle's micro-gradients, laid out like flat_g; exists only while accum_steps > 1.  Never zeroed: the first
        micro-step of a cycle overwrites it"""
        if self.acc is None:
            self.acc = torch.empty_like(self.flat_g)
        return self.acc

    @torch.no_grad()
    def _accumulate(self, lo, hi, final):
        """micro-steps 1 .. k-1: acc[lo:hi] (+)= flat_g[lo:hi]; micro-step k: flat_g[lo:hi] = (acc + flat_g) / k and, on the bf16 wire,
        its image in comm[lo:hi] (over the micro-gradient's image the stage graph left there).  HIP pass on the GPU; torch on the CPU
        test path, same statement order"""
        g, acc = self.flat_g[lo:hi], self._accumulator()[lo:hi]
        wire = self.comm[lo:hi] if (final and self.comm is not None) else None
        scale = 1.0 / self._accum_steps
        if self.fused and g.is_cuda:
            st = torch.cuda.current_stream().cuda_stream
            if final:
                lib.call("adnm_grad_accum_final", acc.data_ptr(), g.data_ptr(), None if wire is None else wire.data_ptr(), hi - lo, scale, st)
            else:
                lib.call("adnm_grad_accum", acc.data_ptr(), g.data_ptr(), hi - lo, int(self._micro == 0), st)
        elif final:
            g.copy_((acc + g) * scale)
            if wire is not None:
                wire.copy_(g.to(torch.bfloat16))
        elif self._micro == 0:
            acc.copy_(g)
        else:
            acc.add_(g)

    def _bucket_ready(self, j, pending, cast_done=False):
        """bucket j of this pass is complete.  accum_steps == 1: start its all-reduce.  k > 1: fold it into the accumulator first — right
        here, so that on the last micro-step bucket j's averaged gradient goes on the wire while the earlier stages' backward still
        runs — and start the all-reduce on the last micro-step only"""
        lo, hi = self.buckets[j]
        if self._accum_steps > 1 and hi > lo:
            final = self._micro == self._accum_steps - 1
            self._accumulate(lo, hi, final)
            if not final:
                return
            cast_done = cast_done or self.comm is not None   # (the final pass wrote the wire image itself)
        self._reduce_begin(lo, hi, pending, cast_done=cast_done)

    # ------------------------------------------------------------------ one-time setup
    def _fwd_bwd(self, x, tgt):
        ops.GRADS.reset_claims(id(self))
        out = self.model(x)
        loss = self.loss_fn(out, tgt)
        with self._deferred():   # the second-stage folds of the parameter gradients: batched, flushed on the way out
            loss.backward()
        return loss

    def _deferred(self):
        """the context of a backward pass: second-stage folds of the parameter gradients batched (ops.FOLDS), flushed on the way out"""
        on = self.defer_folds and self.used is not None and self.flat_g.is_cuda
        dev = self.flat_g.device if self.used is not None else torch.device("cpu")
        return ops.FOLDS.active(dev, on)

    @torch.no_grad()
    def _flatten(self):
        used = [p for p in self.model.parameters() if p.requires_grad and p.grad is not None]
        # flat layout = the stages in BACKWARD order (last stage first): every stage's gradients are one contiguous range = one bucket,
        # in the order the buckets become ready.  groups[j] = parameters of the j-th bucket.
        groups = [used]
        if self.staged:
            K = len(self.stage_defs)
            claimed = set().union(*[ids for _, ids in self.stage_defs if ids is not None])
            owners = {}
            for k, (_, ids) in enumerate(self.stage_defs):
                for i in (ids or ()):
                    owners.setdefault(i, []).append(k)
            twice = [n for n, p in self.model.named_parameters() if len(owners.get(id(p), ())) > 1]
            if twice:
                raise RuntimeError(f"FlatTrainer: parameters claimed by more than one stage of forward_stages(): {twice[:8]}")
            catch_all = any(ids is None for _, ids in self.stage_defs)
            groups = []
            for k in range(K - 1, -1, -1):
                ids = self.stage_defs[k][1]
                groups.append([p for p in used if (id(p) in ids if ids is not None else id(p) not in claimed)])
            left = {id(p) for p in used} - {id(p) for g in groups for p in g}
            if left and not catch_all:
                # a parameter no stage names would be asked for in no part's backward(inputs=...): it would never get a gradient and
                # only be weight-decayed — refuse instead of training a model with silently frozen parameters
                names = [n for n, p in self.model.named_parameters() if id(p) in left]
                raise RuntimeError(f"FlatTrainer: parameters that receive gradients but belong to no stage of forward_stages(): {names[:8]}")
            used = [p for g in groups for p in g]
        self.late, self.early = groups[0], [p for g in groups[1:] for p in g]
        dev, dt = used[0].device, used[0].dtype
        # one (lo, hi) bucket PER GROUP, empty groups included (a frozen or parameter-free stage): buckets[j] belongs to backward part j
        offs, total, buckets = [], 0, []
        for g in groups:
            total = (total + 7) // 8 * 8  # a stage boundary is also a bucket boundary of the bf16 wire buffer (16-byte aligned there too)
            lo = total
            for p in g:
                offs.append(total)
                total += (p.numel() + 3) // 4 * 4  # keep every tensor 16-byte aligned inside the flat buffers
            buckets.append((lo, total))
        assert len(buckets) == len(groups) and (not self.staged or len(buckets) == len(self.stage_defs))
        self.groups = groups
        self.flat_p = torch.zeros(total, dtype=dt, device=dev)
        self.flat_g = torch.zeros(total, dtype=dt, device=dev)
        self.exp_avg = torch.zeros(total, dtype=dt, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=dt, device=dev)
        self.state = torch.zeros(4, dtype=torch.float32, device=dev)
        self.g_views = []

        # modules name the weights their NHWC kernels want in (out, kh, kw, in) memory order (dense 3x3 convs, transposed convs)
        nhwc = {id(p) for m in self.model.modules() if hasattr(m, "adnm_nhwc_parameters") for p in m.adnm_nhwc_parameters()}

        def shaped(flat, o, p):
            """view of the flat slice with p's logical shape.  The weights of the dense NHWC convs get channels-last strides: the
            kernels then read them (and write their gradients) as they lie, with the reduction axis contiguous."""
            t = flat[o:o + p.numel()]
            if id(p) in nhwc and p.dim() == 4 and p.is_cuda:
                co, ci, kh, kw = p.shape
                return t.view(co, kh, kw, ci).permute(0, 3, 1, 2)
            return t.view_as(p)
        for p, o in zip(used, offs):
            view = shaped(self.flat_p, o, p)
            view.copy_(p.data)
            p.data = view
            self.g_views.append(shaped(self.flat_g, o, p))
            p.grad = None
        self.used, self.n = used, total
        self.offs = offs
        # gradient buckets in the order they become ready (= the order they are all-reduced); an empty stage has an empty bucket
        # (lo == hi), which _reduce_begin skips
        self.buckets = buckets
        self.n_late = self.buckets[0][1]
        self.group_ranges, lo = [], 0
        for g in groups:
            self.group_ranges.append((lo, lo + len(g)))
            lo += len(g)
        if self.world > 1 and self.reduce_dtype == "bf16":
            self.comm = torch.empty(total, dtype=torch.bfloat16, device=dev)
        # backward functions that allocate parameter gradients write them straight into these slices (ops.GRADS)
        ops.GRADS.register(id(self), {p.data_ptr(): gv for p, gv in zip(used, self.g_views)})
        if self.fused:
            self.ws = torch.empty(int(lib.query("adnm_adamw_ws_bytes")), dtype=torch.uint8, device=dev)
        if self._accum_steps > 1:
            self._accumulator()
        if self.monitor:
            self._stats_block()
        if self.ema_decay is not None:   # starts as a copy of the parameters (padding included: zero, and zero it stays)
            self.ema = self.flat_p.clone()
            self._ema_info = torch.zeros(2, dtype=torch.float32, device=dev)
        if self._pending is not None:   # a state loaded before the first backward: now there is a layout to write it into
            sd, self._pending = self._pending, None
            self._apply_state(sd, quant=False, ema=self._pending_ema)

    def bucket_report(self):
        """[(bucket index in all-reduce order, first element, last element + 1, bytes on the wire)]: what each stage's collective moves —
        the sizes to price against the xGMI ring."""
        eb = 2 if self.reduce_dtype == "bf16" else 4
        return [(j, lo, hi, (hi - lo) * eb) for j, (lo, hi) in enumerate(self.buckets)]

    def _setup_shadows(self, mode):
        """The narrow SHADOW of the flat parameter buffer (ops.ShadowRegistry / ops.ShadowSet; include/adnm_hip.h: adnm_adamw_step): mode 1 =
        bf16, 2 = per-tensor scaled e4m3 (weight records in ops.QUANT's table, one per matrix-shaped parameter), rewritten by every
        optimiser pass.  The weight-streaming GEMMs read it instead of the fp32 values.  mode 0 (exact fp32, CPU, ADNM_NARROW_WEIGHTS=0): none."""
        self.shadow, self.shadow_mode, self._shadow = None, 0, None
        import os
        if mode == 0 or not self.fused or not self.flat_p.is_cuda or os.environ.get("ADNM_NARROW_WEIGHTS", "1") == "0":
            return
        dev = self.flat_p.device
        self.shadow_mode = mode
        self.shadow = torch.zeros(self.n, dtype=torch.bfloat16 if mode == 1 else torch.uint8, device=dev)
        rows = []
        for p in self.used:   # fp8: a record per GEMM-shaped weight (every other tensor: no scale, its shadow bytes are never read)
            rows.append(ops.QUANT.weight_row(dev, p.data_ptr()) if (mode == 2 and p.dim() >= 2 and p.numel() >= 1024) else -1)
        self._shadow = ops.ShadowSet(self.flat_p, self.shadow, mode, self.offs, rows, self.used)
        self.seg_end, self.seg_rec = self._shadow.seg_end, self._shadow.seg_rec
        ops.SHADOWS.register(id(self), self._shadow)

    def refresh_shadows(self, collect_only=False):
        """Rewrite the narrow shadow from the parameters as they are.  step(), the eager GEMMs' shadow lookups and GraphedForward do this
        by themselves after every write torch can see (load_state_dict / checkpoint.load_reference_checkpoint, an in-place op on a
        parameter or a view of it, a write through flat_p: ops.ShadowSet); call it after a write torch cannot see — through p.data, a raw
        device pointer, a DLPack alias — before the next forward or step.  fp8: first re-derives the scale_b of every WEIGHT record from
        max |w| as it is now (adnm_quant_update's formula), so that new weights are not quantised with the old weights' scales (and
        saturate at 448); the activation / gradient records stay on their delayed-scaling schedule.  Not inside a hipGraph capture.
        collect_only (fp8, prepare's first calibration): only gather max |w| per weight record."""
        if self._shadow is None:
            return
        if collect_only:
            self._shadow.write(collect_only=True)
        else:
            self._shadow.refresh()

    def _release_captures(self):
        """What the captures own, given back in a fixed order: the graphs first, the tail before the stage graphs before the first (they
        reference graph-pool memory), then the tensors that live in that pool (the static loss with its autograd graph, the stage
        hand-over, the static inputs, the tail's hyper-parameters), then the split-K scope the graphs' launches point into, then the
        pin on the fp8 table; last the gradient accumulator (no graph points into it; a step after a failed prepare() makes a new one)
        and the statistics block of a monitored run (the tail graph, gone by then, held its address; its counts end with the captures).
        The only such list: close() and a failed prepare() both end here."""
        self.tail = None
        self.graphs = []
        self.graph2 = None
        self.graph = None
        self.static_loss = None
        self._carry = self._cuts = None
        self.sx = self.st = None
        self._feed = None   # (step_from's checked feed: checked against THESE static buffers)
        self.hyper = self._hyper_host = None
        self._splitws = None
        pin, self._pin = self._pin, None
        if pin is not None:
            pin.release()
        self.acc = None
        self._micro = 0
        self._stats = None

    def close(self):
        """Give back everything this trainer owns on the device, in a fixed order, NOW (not whenever the cyclic collector gets to
        it): what the captures own (_release_captures), then the shadow and gradient-destination registrations.  Idempotent;
        __del__ calls it.  A round-2 run aborted (rc 134) because dead trainers of failed tests — kept alive by their tracebacks —
        were finalised by the cyclic GC in the middle of a NEW trainer's warm-up / stream capture: destroying a hipGraph (and
        freeing its private pool) while another capture is in flight on the device is not allowed by the runtime.  prepare()
        therefore also collects BEFORE it starts and keeps the collector off until the last capture has ended."""
        self._release_captures()
        try:
            ops.SHADOWS.drop(id(self))
        except Exception:
            pass
        try:
            ops.GRADS.drop(id(self))   # lock-free for a finaliser: queued, drained by the next register / take
        except Exception:
            pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _gather(self, lo=0, hi=None):
        """Copy the gradients of used[lo:hi] that were not born inside the flat buffer (same data_ptr = already in place)."""
        hi = len(self.used) if hi is None else hi
        # a slice that ONE backward node claimed holds that gradient itself (whatever tensor object autograd kept for p.grad)
        born = ops.GRADS.born_in_place(id(self))
        pairs = [(gv, p.grad) for gv, p in zip(self.g_views[lo:hi], self.used[lo:hi])
                 if p.grad is not None and p.grad.data_ptr() != gv.data_ptr() and p.data_ptr() not in born]
        self.gathered = [i for i, (gv, p) in enumerate(zip(self.g_views[lo:hi], self.used[lo:hi]), lo)
                         if p.grad is not None and p.grad.data_ptr() != gv.data_ptr() and p.data_ptr() not in born]   # (tools/gather_report.py)
        if pairs:
            torch._foreach_copy_([d for d, _ in pairs], [s for _, s in pairs])

    # staged backward.  part 0 = the whole forward + the backward of the LAST stage (down to its input cut); part j = the backward of
    # stage K-1-j, started from the gradients the part before left at its output cut.
    def _stage_part0(self, x, tgt):
        ops.GRADS.reset_claims(id(self))
        K = len(self.stage_defs)
        self._cuts = [None] * K   # stage k >= 1: (tensors the stage before produced, their detached twins)
        args = (x,)
        for k, (fn, _) in enumerate(self.stage_defs):
            if k > 0:
                # a true cut: the stage runs on detached twins, so a later stage's backward stops there (a skip tensor also reaches the
                # loss THROUGH later layers of its own stage; that path belongs to the earlier part, which starts from the originals
                # with the twins' gradients)
                twins, origs, targs = {}, [], []
                for t in args:
                    if torch.is_tensor(t) and t.requires_grad:
                        if id(t) not in twins:   # a tensor handed over twice gets one twin: its gradient is the sum over both uses
                            twins[id(t)] = t.detach().requires_grad_(True)
                            origs.append(t)
                        targs.append(twins[id(t)])
                    else:
                        targs.append(t)
                self._cuts[k] = (origs, [twins[id(t)] for t in origs])
                args = tuple(targs)
            args = fn(*args)
            args = args if isinstance(args, tuple) else (args,)
        loss = self.loss_fn(args[0], tgt)
        self._backward_stage(K - 1, [loss], None)
        return loss

    def _backward_stage(self, k, roots, grads):
        """backward of stage k from `roots` (the loss, or the stage's outputs with the gradients carried over the cut) down to its own
        parameters and the twins at its input cut; leaves the twins' gradients as the next part's carry"""
        twins = self._cuts[k][1] if k > 0 else []
        # backward(inputs=...) accumulates through the ordinary AccumulateGrad path (which keeps a fresh gradient without copying it;
        # autograd.grad() was measured to cost ~290 extra device copies per step here)
        for t in twins:
            t.grad = None
        j = len(self.stage_defs) - 1 - k
        wanted = self.groups[j] + twins
        if wanted and roots:   # (a frozen FIRST stage has neither parameters nor an input cut: nothing to differentiate)
            with self._deferred():
                torch.autograd.backward(roots, grad_tensors=grads, inputs=wanted)
        self._carry = [(o, tw.grad) for o, tw in zip(self._cuts[k][0], twins) if tw.grad is not None] if k > 0 else []
        self._gather(*self.group_ranges[j])

    def _stage_part(self, j):
        k = len(self.stage_defs) - 1 - j
        self._backward_stage(k, [t for t, _ in self._carry], [g for _, g in self._carry])

    def prepare(self, x, tgt):
        """Dry-run backward (finds the parameters that receive gradients), flatten, and capture the graph(s).
        Ownership: objects with device-side destructors that died earlier (old trainers, graphs of failed runs) are collected
        BEFORE anything starts, and the cyclic collector stays off until the last capture has ended (see close()); an exception
        on the way — inside a capture included — unbinds the fold queue, drops the half-built graphs and re-raises."""
        self._not_under_ema("prepare")
        gc.collect()
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            self._prepare(x, tgt)
        except BaseException:
            self._abort_prepare()
            raise
        finally:
            if gc_was_on:
                gc.enable()

    def _abort_prepare(self):
        """After an exception in prepare(): torch.cuda.graph's __exit__ has already ended a capture in flight; what is left is
        OUR state — the thread's fold-queue binding (a kernel wrapper may have died between bind and unbind), the deferral
        switch of this device, and what the captures own (_release_captures), which must not survive half-captured."""
        try:
            lib.load().adnm_foldq_bind(None)
        except Exception:
            pass
        dev = self.flat_g.device if self.flat_g is not None else None
        if dev is not None and dev.type == "cuda":
            try:
                ops.FOLDS.abort(dev)
            except Exception:
                pass
        self._release_captures()

    def _prepare(self, x, tgt):
        self.model.zero_grad(set_to_none=True)
        # fp8 (BASELINE config 5): the dry run and the calibration step run on bf16 operands; the calibration step — after the
        # parameters have moved into the flat buffer, so that the call-site keys are the final addresses — collects every GEMM
        # operand's amax, from which adnm_quant_update makes the first scales.  From then on the steps run on fp8 operands and
        # re-calibrate themselves every ops.QUANT.period steps (delayed per-tensor scaling, all on the device: graph-replayable).
        self.fp8 = ops.mfma_precision() == "fp8" and x.is_cuda
        if self.fp8:
            ops.set_mfma_precision("bf16")
        try:
            self._fwd_bwd(x, tgt)
            self._flatten()
            if self.fp8:
                ops.QUANT.reset(x.device)
                self._setup_shadows(2)                        # weight records (after the reset: it may forget the keys)
                self.refresh_shadows(collect_only=True)      # max |w| of every GEMM weight
                ops.QUANT.calibrating = True
                for p in self.used:
                    p.grad = None
                self._run_eager(x, tgt)                       # bf16 operands, fp32 weights: every call site's activation / gradient maxima
                ops.QUANT.calibrating = False
                ops.QUANT.update(x.device)                    # -> the first scales, weights included
                self._shadow.write()                          # the e4m3 shadow, written with them
                for p in self.used:
                    p.grad = None
            else:
                self._setup_shadows(1 if (x.is_cuda and ops.mfma_precision() == "bf16") else 0)
                self.refresh_shadows()
        finally:
            ops.QUANT.calibrating = False
            if self.fp8:
                ops.set_mfma_precision("fp8")
        if self._pending_quant is not None:   # (the calibration above made the rows; the captures below read the loaded scales)
            q, self._pending_quant = self._pending_quant, None
            if self.fp8:
                self._load_quant(q)
                self._shadow.write()
                self._shadow.mark_current()
        if not self.use_graph:
            return
        self.sx, self.st = x.clone(), tgt.clone()

        def eager():
            for p in self.used:
                p.grad = None
            self._run_eager(self.sx, self.st)
        ops.warm_up(eager, 2)
        torch.cuda.synchronize()
        for p in self.used:
            p.grad = None
        self.graph = torch.cuda.CUDAGraph()
        # what the graphs hold besides torch's pool: the uncached [arrival counters | slabs] region of their split GEMM launches (one
        # scope for all of this trainer's graphs: they replay one after the other on one stream) and, in the fp8 configuration, pointers
        # into the device's quantisation table (pinned: a later calibration re-uses the rows instead of re-assigning them)
        self._splitws = ops.SPLITWS.open_scope(x.device)
        if self.fp8 and self._pin is None:
            self._pin = ops.QUANT.pinned(x.device)

        def grab(g, body, *args, pool=None):
            # thread_local: RCCL's watchdog thread may query events while we capture; only this thread's calls are checked
            return ops.capture(g, lambda: body(*args), self._splitws, pool=pool, capture_error_mode="thread_local")

        def part(j):
            # each stage graph ends with the wire cast of ITS bucket (bf16 wire): a step at N > 1 is then K graph replays + K collective
            # calls + the tail graph below, nothing else is launched from the host
            loss = self._stage_part0(self.sx, self.st) if j == 0 else self._stage_part(j)
            self._wire_cast(j)
            return loss
        self.graphs, self.graph2, self.tail = [], None, None
        if not self.staged:
            self.static_loss = grab(self.graph, self._run_eager, self.sx, self.st)   # forward, backward, gather
            return
        self.static_loss = grab(self.graph, part, 0)
        for j in range(1, len(self.stage_defs)):   # same memory pool: every part reads what the parts before saved for it
            g = torch.cuda.CUDAGraph()
            grab(g, part, j, pool=self.graph.pool())
            self.graphs.append(g)
        self.graph2 = self.graphs[0] if self.graphs else None
        if not self.fused:
            return
        # the tail of a step: (bf16 wire: averages back to fp32) -> fp8 scale update -> clip + AdamW (+ shadow), with the learning rate and
        # the clip threshold in device memory (self.hyper) so that the captured launches follow the host's schedules
        self.hyper = torch.tensor([self.lr, self.max_norm], dtype=torch.float32, device=x.device)
        self._hyper_host = (float(self.lr), float(self.max_norm))
        # (the statistics block of a monitored run among them: the warm-up's guard counted one step, prepare() leaves the block zero)
        # (and the average with its two floats: adnm_ema_update's first launch happens in this warm-up, not inside the capture)
        live = [t for t in (self.flat_p, self.exp_avg, self.exp_avg_sq, self.state, self.flat_g, self.shadow, self._stats, self.ema,
                            self._ema_info) if t is not None]
        keep = [t.clone() for t in live]
        qsave = ops.QUANT.snapshot(x.device) if self.fp8 else None
        try:
            ops.warm_up(self._tail_body, 1)
            self.tail = torch.cuda.CUDAGraph()
            grab(self.tail, self._tail_body, pool=self.graph.pool())
        finally:
            # the warm-up advanced the optimiser once: put everything back, also when the warm-up or the capture raised (should the
            # restore itself fail, its exception carries the first one as __context__)
            for dst, src in zip(live, keep):
                dst.copy_(src)
            if qsave is not None:
                ops.QUANT.restore(x.device, qsave)
            if self._shadow is not None:   # (parameters and shadow restored together: the copy moved flat_p's version counter)
                self._shadow.mark_current()

    def _wire_cast(self, j):
        """fp32 -> bf16 copy of bucket j into the wire buffer (captured at the end of stage graph j)"""
        if self.world > 1 and self.reduce_dtype == "bf16":
            lo, hi = self.buckets[j]
            if hi > lo:
                self._cast(self.flat_g[lo:hi], self.comm[lo:hi])

    def _tail_body(self):
        if self.world > 1 and self.reduce_dtype == "bf16":
            for lo, hi in self.buckets:
                if hi > lo:
                    self._cast(self.comm[lo:hi], self.flat_g[lo:hi], 1.0 / self.world)
        self._update(hyper=True)

    def _update(self, hyper=False):
        """the end of a step, on gradients that are final: (monitor: guard + statistics ->) fp8 table update -> clip + AdamW (+ shadow)
        (-> the moving average of the parameters).  Eagerly and as the body of the tail graph.
        monitor, more than one rank: the guard runs AFTER the all-reduce, on a flat_g that holds the same bits on every rank (the
        collective leaves one result everywhere — fp32 sums and, on the bf16 wire, the bf16 sums every rank casts back with the same
        kernel), so every rank takes the same decision from the same state[1]: the ranks skip or apply together without exchanging
        a flag (tests/test_step_guard_gloo.py)."""
        guard = None
        if self.monitor:
            self._guard(hyper)
            guard = self._stats
        if self.fp8:
            # one launch: amax -> scales on calibration steps, the next step's record flags.  BEFORE the optimiser pass: that pass writes
            # the e4m3 shadow of the updated weights with the scales the next step's GEMMs will read
            ops.QUANT.update(self.flat_g.device, guard=guard)
        self._optimizer_step(hyper=hyper)
        if self.ema is not None:
            self._ema_update()

    def _run_eager(self, x, tgt, between=None):
        """between(j): called after part j (its bucket is complete) while parts remain — the N > 1 flow starts the bucket's all-reduce there"""
        if not self.staged:
            loss = self._fwd_bwd(x, tgt)
            self._gather()
            return loss
        loss = self._stage_part0(x, tgt)
        for j in range(1, len(self.stage_defs)):
            if between is not None:
                between(j - 1)
            self._stage_part(j)
        return loss

    # ------------------------------------------------------------------ the collective
    def _cast(self, src, dst, scale=1.0):
        """fp32 <-> bf16 copy of a gradient range (HIP pass on the GPU; torch on the CPU test path)."""
        if self.fused and src.is_cuda:
            name = "adnm_cast_f32_bf16" if src.dtype == torch.float32 else "adnm_cast_bf16_f32"
            lib.call(name, src.data_ptr(), dst.data_ptr(), src.numel(), float(scale), torch.cuda.current_stream().cuda_stream)
        else:
            dst.copy_(src.to(dst.dtype) if scale == 1.0 else (src.float() * scale).to(dst.dtype))

    def _reduce_begin(self, lo, hi, pending, cast_done=False):
        """Start averaging flat_g[lo:hi] over the ranks.  RCCL: asynchronously on its own stream (it first waits for what the
        compute stream has enqueued so far, i.e. the graph that produced the range), so the next graph runs beside the ring."""
        if self.world == 1 or hi <= lo:
            return
        nccl = dist.get_backend(self.group) == "nccl"
        if self.reduce_dtype == "bf16":
            t = self.comm[lo:hi]
            if not cast_done:   # (the stage graphs end with their bucket's cast)
                self._cast(self.flat_g[lo:hi], t)
            op = dist.ReduceOp.SUM
        else:
            t = self.flat_g[lo:hi]
            op = dist.ReduceOp.AVG if nccl else dist.ReduceOp.SUM
        work = dist.all_reduce(t, op=op, group=self.group, async_op=True)
        pending.append((work, lo, hi, nccl))

    def _reduce_end(self, pending, tail=False):
        """tail: the casts back / the division are part of the captured tail graph"""
        for work, lo, hi, nccl in pending:
            work.wait()   # the compute stream waits for the ring; the host does not block (RCCL)
            if tail and self.reduce_dtype == "bf16":
                continue
            if self.reduce_dtype == "bf16":
                self._cast(self.comm[lo:hi], self.flat_g[lo:hi], 1.0 / self.world)
            elif not nccl:
                self.flat_g[lo:hi].div_(self.world)

    # ------------------------------------------------------------------ per step
    def step(self, x, tgt, eager=False):
        """One training step.  eager=True launches the same work without the captured graphs (bench.py's instrumented steps:
        per-launch HIP events cannot be recorded inside a graph replay).
        accum_steps = k > 1: one MICRO-step; returns this micro-batch's loss.  Calls 1 .. k-1 of a cycle run forward and backward and
        add every bucket into the accumulator: no collective, no fp8 table update, no optimiser pass.  Call k adds its own gradient,
        leaves the mean of the k gradients in flat_g and goes on exactly like a plain step (all-reduce, clip, AdamW, shadow).
        monitor=True: every call adds its loss to the statistics; the optimiser step (once per cycle, on the averaged gradient — a
        non-finite micro-gradient reaches it through the accumulator) is skipped when that gradient is not finite.  A skipped cycle ends
        like any other: micro_step is 0 again and the next cycle overwrites the accumulator."""
        self._not_under_ema("step")
        if self.used is None:
            self.prepare(x, tgt)
        elif self._shadow is not None and self._shadow.stale():   # a write outside the optimiser (a checkpoint load, an in-place op)
            self._shadow.refresh()
        pending = []
        nb = len(self.buckets)
        graphed = False
        if self.graph is not None and not eager:
            if x.data_ptr() != self.sx.data_ptr():
                self.sx.copy_(x, non_blocking=True)
                self.st.copy_(tgt, non_blocking=True)
            self.graph.replay()
            self._bucket_ready(0, pending, cast_done=self.staged)
            if self.staged:
                for j, g in enumerate(self.graphs, start=1):
                    g.replay()
                    if j < nb:
                        self._bucket_ready(j, pending, cast_done=True)
            loss = self.static_loss
            graphed = True
        else:
            for p in self.used:
                p.grad = None
            if self.staged:
                loss = self._run_eager(x, tgt, between=lambda j: self._bucket_ready(j, pending))
                self._bucket_ready(nb - 1, pending)
            else:
                loss = self._run_eager(x, tgt)
                self._bucket_ready(0, pending)
            for p in self.used:
                p.grad = None
        if self.monitor:
            self._loss_stat(loss)
        if self._micro < self._accum_steps - 1:   # a micro-step inside a cycle ends here: parameters, moments, step counter, fp8 table untouched
            self._micro += 1
            return loss
        self._micro = 0
        tail = graphed and self.tail is not None and (self.world == 1 or self.reduce_dtype == "bf16" or dist.get_backend(self.group) == "nccl")
        self._reduce_end(pending, tail=tail)
        if tail:
            if (float(self.lr), float(self.max_norm)) != self._hyper_host:   # a schedule moved them: two floats to the device
                self._hyper_host = (float(self.lr), float(self.max_norm))
                self.hyper.copy_(torch.tensor(self._hyper_host, dtype=torch.float32), non_blocking=True)
            self.tail.replay()
        else:
            self._update()
        if not self._skip_host:   # (fused: always; the device's own counter, state[0], is the one a skipped step leaves alone)
            self._steps += 1
        return loss

    def step_from(self, feed, eager=False):
        """step() on the next batch of a dataio.ResidentDataset; returns what step() returns.  Prepared with graphs: ONE launch writes the
        batch into the static buffers the graphs read (self.sx / self.st) and step() runs on them, so that its pointer test skips both
        copies.  The first call (it prepares), use_graph=False and eager=True fetch into tensors of their own.  With accum_steps = k
        every micro-step takes the feed's next batch."""
        self._not_under_ema("step_from")
        if self.graph is None or eager:
            x, tgt = feed.fetch()
            return self.step(x, tgt, eager=eager)
        if self._feed is None or self._feed() is not feed:   # once per feed: the static buffers are what the feed writes
            if tuple(self.sx.shape) != tuple(feed.x_shape) or tuple(self.st.shape) != tuple(feed.tgt_shape) or self.sx.device != feed.device:
                raise RuntimeError(f"FlatTrainer.step_from: prepared for x {tuple(self.sx.shape)} / tgt {tuple(self.st.shape)} on {self.sx.device}, the "
                                   f"feed gives {tuple(feed.x_shape)} / {tuple(feed.tgt_shape)} on {feed.device}")
            feed._check(self.sx, feed.x_shape, "the trainer's static input")
            feed._check(self.st, feed.tgt_shape, "the trainer's static target")
            self._feed = weakref.ref(feed)
        feed._launch(self.sx, self.st)
        return self.step(self.sx, self.st)

    # ------------------------------------------------------------------ monitor=True: statistics and the skipped step
    STAT_FIELDS = ("steps", "skipped", "norm_sum", "norm_max", "last_norm", "clip_count", "loss_sum", "loss_nonfinite")

    def _stats_block(self):
        """nine doubles laid out as adnm_step_guard documents them (eight statistics, then the skip flag as an int); zero at birth"""
        if self._stats is None:
            self._stats = torch.zeros(9, dtype=torch.float64, device=self.flat_g.device)
        return self._stats

    def _require_monitor(self, what):
        if not self.monitor:
            raise RuntimeError(f"FlatTrainer.{what}: this trainer was built with monitor=False and keeps no statistics; build it with monitor=True")

    def stats(self, reset=False):
        """The statistics since the last reset, as a dict: steps (optimiser steps applied), skipped (steps whose gradient was not
        finite), loss_sum / loss_nonfinite (over every step() call, micro-steps included; this rank's batches), norm_sum / norm_mean /
        norm_max (pre-clip gradient norms of the applied steps — norm_mean is train.py:148's avg_grad_norm), last_norm (of the last step,
        applied or skipped), clip_count / clip_rate (applied steps with max_norm > 0 and norm > max_norm, train.py:142).
        SYNCHRONISES: one device -> host copy that waits for every step enqueued so far.  Meant to be called once per epoch.
        reset=True: reset_stats() afterwards."""
        self._require_monitor("stats")
        vals = self._stats[:8].tolist() if self._stats is not None else [0.0] * 8   # (no step yet / closed: nothing counted)
        d = dict(zip(self.STAT_FIELDS, vals))
        for k in ("steps", "skipped", "clip_count", "loss_nonfinite"):
            d[k] = int(d[k])
        d["norm_mean"] = d["norm_sum"] / d["steps"] if d["steps"] else 0.0
        d["clip_rate"] = d["clip_count"] / d["steps"] if d["steps"] else 0.0
        if reset:
            self.reset_stats()
        return d

    def reset_stats(self):
        """zero the statistics (one memset on the compute stream, behind the steps enqueued so far; no synchronisation)"""
        self._require_monitor("reset_stats")
        if self._stats is not None:
            self._stats.zero_()

    @torch.no_grad()
    def _loss_stat(self, loss):
        """loss_sum += loss (finite) or loss_nonfinite += 1: one eager one-lane launch behind the forward / backward, outside the
        stage graphs; torch on the CPU test path"""
        s = self._stats_block()
        if self.fused and s.is_cuda:
            l = loss.detach()
            if l.dtype != torch.float32 or l.numel() != 1 or not l.is_cuda:
                raise RuntimeError(f"FlatTrainer(monitor=True): the loss must be one fp32 value on the GPU, got {l.dtype} {tuple(l.shape)} on {l.device}")
            lib.call("adnm_loss_stat", l.data_ptr(), s.data_ptr(), torch.cuda.current_stream().cuda_stream)
            return
        v = float(loss)
        if v == v and abs(v) != float("inf"):
            s[6] += v
        else:
            s[7] += 1

    @torch.no_grad()
    def _guard(self, hyper=False):
        """sum of squares of the final gradient -> state[1], the decision skip = not finite, the counters (adnm_step_guard); the same
        statements in torch on the CPU test path, where the decision is a host bool"""
        s = self._stats_block()
        if self.fused:
            lib.call("adnm_step_guard", self.flat_g.data_ptr(), self.n, self.state.data_ptr(), float(self.max_norm),
                     self.hyper.data_ptr() if hyper else None, self.ws.data_ptr(), self.ws.numel(), s.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
            return
        self._norm_host = self.flat_g.norm()
        norm = float(self._norm_host)
        s[4] = norm
        self._skip_host = not (norm == norm and norm != float("inf"))
        if self._skip_host:
            s[1] += 1
            return
        s[0] += 1
        s[2] += norm
        s[3] = max(float(s[3]), norm)
        max_norm = float(torch.tensor(self.max_norm, dtype=torch.float32))   # (the kernel compares in fp32)
        if max_norm > 0 and norm > max_norm:
            s[5] += 1

    # ------------------------------------------------------------------ ema_decay: the moving average of the parameters
    @staticmethod
    def _check_ema_decay(d):
        if d is None:
            return None
        if isinstance(d, bool) or not isinstance(d, (int, float)) or not 0.0 <= float(d) <= 1.0:
            raise ValueError(f"FlatTrainer: ema_decay={d!r} must be None or a number in [0, 1]")
        return float(d)

    def _require_ema(self, what):
        if self.ema_decay is None:
            raise RuntimeError(f"FlatTrainer.{what}: this trainer was built without ema_decay and keeps no average of the weights")

    def _not_under_ema(self, what):
        if self._ema_open:
            raise RuntimeError(f"FlatTrainer.{what}: not inside ema_weights() (the parameters hold the averaged weights; leave the context first)")

    @torch.no_grad()
    def _ema_update(self):
        """ema = d * ema + (1 - d) * p behind the optimiser pass (adnm_ema_update; d from the device's step counter); the same statement
        in torch on the CPU test path, where the step counter is the host's"""
        if self.fused:
            lib.call("adnm_ema_update", self.flat_p.data_ptr(), self.ema.data_ptr(), self.n, self.state.data_ptr(), self.ema_decay,
                     int(self.ema_warmup), self._ema_info.data_ptr(), self._stats.data_ptr() if self.monitor else None,
                     torch.cuda.current_stream().cuda_stream)
        elif not self._skip_host:
            self._torch_ema_for_tests()

    @torch.no_grad()
    def _torch_ema_for_tests(self):
        """adnm_ema_update in torch ops, for the CPU (gloo) tests: d and w in fp32, w * p rounded to fp32, then d * ema + (w * p) formed
        in fp64 (the product is exact there) and rounded once: the kernel's fmaf"""
        d = torch.tensor(self.ema_decay, dtype=torch.float32)
        if self.ema_warmup:
            t = torch.tensor(float(self._steps + 1), dtype=torch.float32)   # (the step this update belongs to: state[0] on the device)
            d = torch.minimum(d, (1.0 + t) / (10.0 + t))
        w = 1.0 - d
        wp = self.flat_p * w.to(self.flat_p.device)
        self.ema.copy_((self.ema.double() * float(d) + wp.double()).float())
        self._ema_info[0] = d
        self._ema_info[1] += 1

    def ema_info(self):
        """{"decay": the d the last update used (0.0 before the first), "updates": updates applied}.  SYNCHRONISES: one small device ->
        host read that waits for every step enqueued so far."""
        self._require_ema("ema_info")
        v = self._ema_info.tolist() if self._ema_info is not None else [0.0, 0.0]   # (no step yet: nothing applied)
        return {"decay": v[0], "updates": int(v[1])}

    @torch.no_grad()
    def _ema_swap(self):
        if self.fused:
            lib.call("adnm_ema_swap", self.flat_p.data_ptr(), self.ema.data_ptr(), self.n, torch.cuda.current_stream().cuda_stream)
        else:
            keep = self.flat_p.clone()
            self.flat_p.copy_(self.ema)
            self.ema.copy_(keep)

    @contextlib.contextmanager
    def ema_weights(self):
        """with trainer.ema_weights(): the model computes with the averaged weights — model.state_dict(), checkpoint.save_reference_checkpoint,
        Validator.step / step_from, Forecaster, eager forwards and GraphedForward graphs captured before (no pointer moves) — and the run
        goes on afterwards as if nothing had happened.  Entry: (fp8: the quantisation table is saved,) flat_p and ema exchange their
        contents in one HIP pass, the narrow shadow is rewritten from the parameters as they now are (fp8: weight scales re-derived).
        Exit, also after an exception: exchanged back, (fp8: the table restored,) the shadow written from the restored parameters with
        the restored scales: flat_p, the shadow and the table are bit for bit what they were.  The raw HIP writes move none of torch's
        version counters, so both ends rewrite the shadow themselves.  Between steps only: not inside a capture, not with an
        accumulation cycle open; step(), step_from(), prepare(), state_dict(), load_state_dict(), snapshot() and a nested ema_weights()
        raise inside."""
        self._require_ema("ema_weights")
        self._require_state("ema_weights")
        self._not_under_ema("ema_weights")
        if self._micro != 0:
            raise RuntimeError(f"FlatTrainer.ema_weights: an accumulation cycle is open (micro-step {self._micro} of {self._accum_steps}); "
                               "finish it first")
        dev = self.flat_p.device
        qsave = ops.QUANT.snapshot(dev) if self.fp8 else None
        self._ema_swap()
        self._ema_open = True
        try:
            if self._shadow is not None:
                self._shadow.refresh()
            yield self
        finally:
            try:
                self._ema_swap()
                if qsave is not None:
                    ops.QUANT.restore(dev, qsave)
                if self._shadow is not None:
                    self._shadow.write()
                    if qsave is not None:   # (the shadow pass collects max |w| into the records whose flag is set: the table once more)
                        ops.QUANT.restore(dev, qsave)
                    self._shadow.mark_current()
            finally:
                self._ema_open = False

    def _optimizer_step(self, hyper=False):
        if self.fused:
            mode = self.shadow_mode
            sh = (self.shadow.data_ptr(), mode, self.seg_end.data_ptr(), self.seg_rec.data_ptr(), self.seg_end.numel(),
                  ops.QUANT.table_ptr(self.flat_p.device) if mode == 2 else None) if mode else (None, 0, None, None, 0, None)
            if self.monitor:   # the norm is the guard's; every kernel returns at entry when the guard set the skip flag
                lib.call("adnm_adamw_step_guarded", self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.exp_avg.data_ptr(),
                         self.exp_avg_sq.data_ptr(), self.n, self.state.data_ptr(), float(self.lr), float(self.betas[0]), float(self.betas[1]),
                         float(self.eps), float(self.wd), float(self.max_norm), *sh, self.hyper.data_ptr() if hyper else None,
                         self._stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
                return
            lib.call("adnm_adamw_step", self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.exp_avg.data_ptr(),
                     self.exp_avg_sq.data_ptr(), self.n, self.state.data_ptr(), float(self.lr), float(self.betas[0]), float(self.betas[1]),
                     float(self.eps), float(self.wd), float(self.max_norm), self.ws.data_ptr(), self.ws.numel(), *sh,
                     self.hyper.data_ptr() if hyper else None, torch.cuda.current_stream().cuda_stream)
        elif not self._skip_host:   # (monitor, CPU test path: a skipped step touches nothing, _steps included)
            self._torch_adamw_for_tests(self._norm_host if self.monitor else None)

    @torch.no_grad()
    def _torch_adamw_for_tests(self, norm=None):
        """Same arithmetic in torch ops — exists only so the CPU (gloo) tests can exercise the N>1 logic and the
        GPU test has an independent statement of the fused kernel's update rule.  bench.py never takes it."""
        g = self.flat_g
        if self.max_norm > 0:
            g = g * torch.clamp(self.max_norm / ((g.norm() if norm is None else norm) + 1e-6), max=1.0)   # (norm: the guard's, formed once)
        step = self._steps + 1
        b1, b2 = self.betas
        self.flat_p.mul_(1 - self.lr * self.wd)
        self.exp_avg.lerp_(g, 1 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (self.exp_avg_sq.sqrt() / (1 - b2 ** step) ** 0.5).add_(self.eps)
        self.flat_p.addcdiv_(self.exp_avg, denom, value=-self.lr / (1 - b1 ** step))

    def grad_norm(self):
        """Pre-clip total gradient norm of the last step (device scalar; train.py:141 reads it with .item()).  monitor=True: of the last
        APPLIED step (a skipped step leaves state alone; stats()["last_norm"] shows its inf / nan)."""
        return self.state[1].sqrt() if self.fused else self.flat_g.norm()

    # ------------------------------------------------------------------ save and resume
    STATE_VERSION = 1

    def _precision(self):
        return "fp8" if self.fp8 else ops.mfma_precision()

    def _used_names(self):
        name_of = {id(p): n for n, p in self.model.named_parameters()}
        return [name_of[id(p)] for p in self.used]

    def _logical(self, host, i):
        """used[i]'s slice of a HOST copy of one flat buffer, seen through the parameter's own layout: logical shape, the strides its
        view into flat_p has (channels-last for the dense-conv weights), no padding"""
        p = self.used[i]
        return host.as_strided(p.shape, p.stride(), self.offs[i])

    def _quant_rows(self):
        """fp8: [(name, row)] of the records of this device's table that belong to this trainer.  A record's key is a weight's data_ptr:
        the name is the parameter whose storage contains it, the offset inside it (when not 0) and the role.  A key inside another
        live trainer's flat buffer is that trainer's; any other key that no parameter of this model contains cannot be named, and
        naming it by guesswork would restore some other call site's scales: NotImplementedError."""
        dev = self.flat_p.device
        keys = ops.QUANT._ent(dev)["keys"]
        lo, params = self.flat_p.data_ptr(), []
        names = self._used_names()
        mine = {id(q) for q in self.used}
        for n, p in self.model.named_parameters():
            if p.device == dev and id(p) not in mine:
                params.append((p.data_ptr(), p.data_ptr() + p.numel() * p.element_size(), n, p.element_size()))
        others = [s for s in ops.SHADOWS.sets(dev) if s is not self._shadow]
        import bisect
        out = []
        for (key, role), row in sorted(keys.items(), key=lambda kv: kv[1]):
            if lo <= key < lo + 4 * self.n:
                off = (key - lo) // 4
                i = bisect.bisect_right(self.offs, off) - 1
                name, inner = names[i], off - self.offs[i]
                if inner >= self.used[i].numel():
                    raise NotImplementedError(f"FlatTrainer.state_dict (fp8): record key of role {role!r} points into the padding behind {name}")
            else:
                hit = [(n, (key - a) // es) for a, b, n, es in params if a <= key < b]
                if not hit:
                    if any(s.lo <= key < s.hi for s in others):
                        continue
                    raise NotImplementedError(f"FlatTrainer.state_dict (fp8): a quantisation record of role {role!r} is keyed by an address "
                                              "that lies in no parameter of this trainer's model; its call site cannot be named")
                name, inner = hit[0]
            out.append((f"{name}|{role}" if inner == 0 else f"{name}+{inner}|{role}", row))
        seen = set()
        for n, _ in out:
            if n in seen:
                raise NotImplementedError(f"FlatTrainer.state_dict (fp8): two quantisation records would both be named {n!r}")
            seen.add(n)
        return out

    def _scalars(self):
        sc = {"version": self.STATE_VERSION, "precision": self._precision(), "steps": int(self._steps), "lr": float(self.lr),
              "max_norm": float(self.max_norm), "betas": (float(self.betas[0]), float(self.betas[1])), "eps": float(self.eps),
              "weight_decay": float(self.wd), "accum_steps": self._accum_steps, "micro_step": self._micro}
        if self.ema_decay is not None:   # (a trainer without the average writes the keys it always wrote, and no others)
            sc["ema_decay"], sc["ema_warmup"] = self.ema_decay, self.ema_warmup
        return sc

    def _live_buffers(self, params=False):
        """the device buffers a saved state is made of (None: this trainer has no such buffer)"""
        open_cycle = self._micro > 0 and self.acc is not None
        bufs = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "state": self.state, "acc": self.acc if open_cycle else None,
                "stats": self._stats if self.monitor else None, "qtab": None, "qstate": None, "ema": self.ema, "ema_info": self._ema_info}
        if params:
            bufs["flat_p"] = self.flat_p
        if self.fp8:
            ent = ops.QUANT._ent(self.flat_p.device)
            bufs["qtab"], bufs["qstate"] = ent["tab"], ent["state"]
        return bufs

    def _pack_state(self, host, scalars, qrows):
        """host: CPU copies of _live_buffers(); -> the layout-independent dict (every tensor owns its memory)"""
        names = self._used_names()
        sd = dict(scalars)
        sd["state_bits"] = host["state"].view(torch.int32).clone()
        per = {}
        for i, name in enumerate(names):
            ent = {k: self._logical(host[k], i).clone(memory_format=torch.contiguous_format) for k in ("exp_avg", "exp_avg_sq")}
            if host["acc"] is not None:
                ent["acc"] = self._logical(host["acc"], i).clone(memory_format=torch.contiguous_format)
            per[name] = ent
        sd["params"] = per
        sd["monitor"] = host["stats"].clone() if host["stats"] is not None else None
        sd["fp8"] = None
        if qrows is not None:
            sd["fp8"] = {"state": host["qstate"].clone(), "rows": {n: host["qtab"][r].clone() for n, r in qrows}}
        if host.get("ema") is not None:
            sd["ema"] = {name: self._logical(host["ema"], i).clone(memory_format=torch.contiguous_format) for i, name in enumerate(names)}
            sd["ema_info"] = host["ema_info"].clone()
        if host.get("flat_p") is not None:
            sd["parameters"] = {name: self._logical(host["flat_p"], i).clone(memory_format=torch.contiguous_format) for i, name in enumerate(names)}
        return sd

    def _require_state(self, what):
        if self.used is None:
            raise RuntimeError(f"FlatTrainer.{what}: the flat buffers do not exist yet (they are laid out by prepare() or the first step())")
        if self.flat_p.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"FlatTrainer.{what}: not inside a hipGraph capture")

    @torch.no_grad()
    def state_dict(self):
        """Everything an interrupted run needs beside model.state_dict(), independent of the flat layout: a plain dict of CPU tensors and
        Python scalars.  "params": {parameter name: {"exp_avg", "exp_avg_sq" (, "acc" while an accumulation cycle is open)}} in the
        parameter's logical shape, contiguous (NCHW for the conv weights the flat buffers hold channels-last), without padding, for the
        parameters that receive gradients; "state_bits": the four floats of `state` as int32; "steps", "lr", "max_norm", "betas", "eps",
        "weight_decay", "accum_steps", "micro_step", "precision", "version"; "monitor": the nine doubles of a monitored trainer or None;
        "fp8": {"state", "rows": {"<parameter name>|<role>": the record's 8 floats}} or None; with ema_decay also "ema": {parameter name: the
        average, in logical shape like the moments}, "ema_info": adnm_ema_update's two floats, "ema_decay", "ema_warmup" (a trainer
        without the average writes none of the four).  SYNCHRONISES: one device -> host copy per
        flat buffer (snapshot() is the form that does not stall the step).  fp8: NotImplementedError when a record of the table cannot
        be named by one of the model's parameters."""
        self._require_state("state_dict")
        self._not_under_ema("state_dict")
        qrows = self._quant_rows() if self.fp8 else None
        host = {k: (None if v is None else v.detach().to("cpu", copy=True)) for k, v in self._live_buffers().items()}
        return self._pack_state(host, self._scalars(), qrows)

    def _check_state(self, sd, strict, ema=True):
        if not isinstance(sd, dict) or sd.get("version") != self.STATE_VERSION or "params" not in sd:
            raise RuntimeError(f"FlatTrainer.load_state_dict: not a trainer state of format version {self.STATE_VERSION} "
                               f"(version: {sd.get('version') if isinstance(sd, dict) else type(sd).__name__!r})")
        if sd["precision"] != self._precision():
            raise RuntimeError(f"FlatTrainer.load_state_dict: the state was saved at matrix-core precision {sd['precision']!r}, this trainer runs "
                               f"at {self._precision()!r}")
        if strict:
            mine = {"betas": (float(self.betas[0]), float(self.betas[1])), "eps": float(self.eps), "weight_decay": float(self.wd)}
            if ema and self.ema_decay is not None and "ema" in sd:
                mine.update(ema_decay=self.ema_decay, ema_warmup=self.ema_warmup)
            bad = [f"{k}: saved {tuple(sd[k]) if k == 'betas' else sd[k]!r}, trainer {v!r}" for k, v in mine.items()
                   if (tuple(sd[k]) if k == "betas" else sd[k]) != v]
            if bad:
                raise RuntimeError("FlatTrainer.load_state_dict: hyper-parameters differ (" + "; ".join(bad) + "); strict=False loads anyway "
                                   "and keeps the trainer's")
        if sd["micro_step"] > 0 and sd["accum_steps"] != self._accum_steps:
            raise RuntimeError(f"FlatTrainer.load_state_dict: the state was saved inside an accumulation cycle (micro-step {sd['micro_step']} of "
                               f"accum_steps={sd['accum_steps']}), this trainer has accum_steps={self._accum_steps}")
        shapes = {n: tuple(p.shape) for n, p in self.model.named_parameters()}
        unknown = sorted(set(sd["params"]) - set(shapes))
        if unknown:
            raise RuntimeError(f"FlatTrainer.load_state_dict: {len(unknown)} names of the state are no parameters of the model, e.g. {unknown[:3]}")
        self._check_shapes(sd, shapes)
        if not ema:
            return
        if strict and self.ema_decay is not None and "ema" not in sd:
            raise RuntimeError("FlatTrainer.load_state_dict: this trainer keeps an average of the weights (ema_decay), the state holds no 'ema'; "
                               "strict=False loads the rest and starts the average anew from the loaded parameters")
        if strict and self.ema_decay is None and "ema" in sd:
            raise RuntimeError("FlatTrainer.load_state_dict: the state holds an average of the weights ('ema'), this trainer was built without "
                               "ema_decay; strict=False ignores it")
        if self.ema_decay is not None and "ema" in sd:
            unknown = sorted(set(sd["ema"]) - set(shapes))
            if unknown:
                raise RuntimeError(f"FlatTrainer.load_state_dict: {len(unknown)} names of the state's 'ema' are no parameters of the model, e.g. {unknown[:3]}")
            for n, t in sd["ema"].items():
                if tuple(t.shape) != shapes[n]:
                    raise RuntimeError(f"FlatTrainer.load_state_dict: ema of {n} has shape {tuple(t.shape)}, the parameter {shapes[n]}")

    @staticmethod
    def _check_shapes(sd, shapes):
        open_cycle = sd["micro_step"] > 0
        for n, ent in sd["params"].items():
            for k in ("exp_avg", "exp_avg_sq") + (("acc",) if open_cycle else ()):
                if k not in ent:
                    raise RuntimeError(f"FlatTrainer.load_state_dict: {n} has no {k!r} in the state")
                if tuple(ent[k].shape) != shapes[n]:
                    raise RuntimeError(f"FlatTrainer.load_state_dict: {k} of {n} has shape {tuple(ent[k].shape)}, the parameter {shapes[n]}")

    @torch.no_grad()
    def load_state_dict(self, sd, strict=True):
        """Take over a state_dict(): moments, `state`, step count, lr and max_norm (they reach the tail graph's device copy with the next
        step), an open accumulation cycle, the monitor block, the fp8 table's rows.  IN PLACE, on the current stream: no buffer moves, so
        the captured graphs of a prepared trainer stay valid.  Any flat layout loads any other: the parameter name is the only key.
        The average of the weights: a state without 'ema' into a trainer with ema_decay raises (strict=False: the average starts anew as a
        copy of the parameters as they are when the state is applied, its counters zero); a state with 'ema' into a trainer without
        raises (strict=False: ignored); another ema_decay / ema_warmup counts as differing hyper-parameters.
        Raises on another set of names or another shape, on other betas / eps / weight_decay (strict=False: the trainer keeps its own),
        on another accum_steps while the saved cycle is open, on another precision, and in fp8 on a record that one side lacks.  The
        parameters themselves are model.state_dict()'s business: load them FIRST (checkpoint.load_training_state does both).
        Before the flat buffers exist (no prepare(), no step yet) the scalars are taken at once and the tensors are kept and written
        when the layout is made; fp8 rows after prepare()'s calibration has created them."""
        self._load(sd, strict)

    def _load(self, sd, strict=True, quant=True, ema=True):
        """ema=False (checkpoint.from_torch_adamw_state): the state has no say about the average; it stays as it is"""
        self._not_under_ema("load_state_dict")
        if self.used is not None and self.flat_p.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FlatTrainer.load_state_dict: not inside a hipGraph capture")
        self._check_state(sd, strict, ema)
        if self.used is None:
            self._take_scalars(sd)
            self._pending, self._pending_quant, self._pending_ema = sd, (sd.get("fp8") if quant else None), ema
            return
        self._apply_state(sd, quant=quant, ema=ema)

    def _take_scalars(self, sd):
        self._steps, self._micro = int(sd["steps"]), int(sd["micro_step"])
        self.lr, self.max_norm = float(sd["lr"]), float(sd["max_norm"])

    def _apply_state(self, sd, quant=True, ema=True):
        names = self._used_names()
        missing, unexpected = sorted(set(names) - set(sd["params"])), sorted(set(sd["params"]) - set(names))
        if missing or unexpected:
            raise RuntimeError(f"FlatTrainer.load_state_dict: the state does not match the parameters this trainer updates: {len(missing)} "
                               f"missing (e.g. {missing[:3]}), {len(unexpected)} unexpected (e.g. {unexpected[:3]})")
        self._check_shapes(sd, {n: tuple(p.shape) for n, p in zip(names, self.used)})
        if quant and self.fp8:
            rows = self._match_quant(sd.get("fp8"))   # (raises before anything is written)
        open_cycle = sd["micro_step"] > 0

        with_ema = ema and self.ema is not None and "ema" in sd
        if with_ema:
            missing, unexpected = sorted(set(names) - set(sd["ema"])), sorted(set(sd["ema"]) - set(names))
            if missing or unexpected:
                raise RuntimeError(f"FlatTrainer.load_state_dict: the state's 'ema' does not match the parameters this trainer updates: "
                                   f"{len(missing)} missing (e.g. {missing[:3]}), {len(unexpected)} unexpected (e.g. {unexpected[:3]})")

        def put(buf, key):
            # one host image of the whole flat buffer (padding zero, as the buffers are born), then ONE copy into the buffer where it is
            host = torch.zeros(self.n, dtype=buf.dtype)
            for i, name in enumerate(names):
                self._logical(host, i).copy_(sd["ema"][name] if key == "ema" else sd["params"][name][key])
            buf.copy_(host)
        put(self.exp_avg, "exp_avg")
        put(self.exp_avg_sq, "exp_avg_sq")
        if open_cycle:
            put(self._accumulator(), "acc")
        self.state.copy_(sd["state_bits"].view(torch.float32))
        if with_ema:
            put(self.ema, "ema")
            self._ema_info.copy_(sd["ema_info"])
        elif ema and self.ema is not None:   # (strict=False, a state without the average: anew from the parameters as they are)
            self.ema.copy_(self.flat_p)
            self._ema_info.zero_()
        if self.monitor and sd.get("monitor") is not None:
            self._stats_block().copy_(sd["monitor"])
        self._take_scalars(sd)
        if quant and self.fp8:
            self._write_quant(sd["fp8"], rows)
        if self._shadow is not None:
            # the shadow of the parameters as they are now, fp8 with the RESTORED scale_b (refresh() would re-derive the weight scales
            # from max |w|: other bits than the interrupted run's)
            self._shadow.write()
            self._shadow.mark_current()

    def _match_quant(self, q):
        if q is None:
            raise RuntimeError("FlatTrainer.load_state_dict: this trainer runs in fp8, the state holds no quantisation table")
        rows = dict(self._quant_rows())
        missing, unexpected = sorted(set(rows) - set(q["rows"])), sorted(set(q["rows"]) - set(rows))
        if missing or unexpected:
            raise RuntimeError(f"FlatTrainer.load_state_dict (fp8): quantisation records differ: {len(missing)} of this trainer are not in the "
                               f"state (e.g. {missing[:3]}), {len(unexpected)} of the state do not exist here (e.g. {unexpected[:3]}); "
                               "prepare() creates the records: call it before the load")
        return rows

    def _write_quant(self, q, rows):
        ent = ops.QUANT._ent(self.flat_p.device)
        host = ent["tab"].cpu()
        for n, r in rows.items():
            host[r] = q["rows"][n]
        ent["tab"].copy_(host)
        ent["state"].copy_(q["state"])

    def _load_quant(self, q):
        self._write_quant(q, self._match_quant(q))

    @torch.no_grad()
    def snapshot(self):
        """A consistent copy of the training state WITHOUT stalling the step: device-to-device copies of flat_p, exp_avg, exp_avg_sq,
        state (and acc, the monitor block, the fp8 table, the average of the weights where they exist) into buffers the snapshot owns, enqueued on the current stream
        behind the steps issued so far, then an event; returns at once.  Call it between steps, outside any capture; read it later with
        TrainerSnapshot.state_dict().  Costs one more copy of the optimiser-sized buffers in device memory while the snapshot lives
        (3 x 4 bytes per parameter: ~0.9 GB for the 72 M parameters of ADNM-UNet; 4 x 4 with ema_decay); nothing is allocated before the
        first call."""
        self._require_state("snapshot")
        self._not_under_ema("snapshot")
        return TrainerSnapshot(self)


class TrainerSnapshot:
    """FlatTrainer.snapshot(): the state as it was between two steps, in device buffers of its own."""

    def __init__(self, tr):
        self._tr = tr
        self._scalars = tr._scalars()
        self._qrows = tr._quant_rows() if tr.fp8 else None
        self._bufs = {}
        for k, v in tr._live_buffers(params=True).items():
            self._bufs[k] = None if v is None else torch.empty_like(v).copy_(v)
        self._event = None
        if tr.flat_p.is_cuda:
            self._event = torch.cuda.Event()
            self._event.record()
        self._sd = None

    @torch.no_grad()
    def state_dict(self):
        """FlatTrainer.state_dict() of the moment the snapshot was taken, plus "parameters": {name: the parameter in logical shape}.
        Waits for the snapshot's event on a side stream, copies to pinned host memory there and synchronises only that stream: the
        training stream is never waited for.  The device buffers are given back after the first call."""
        if self._sd is None:
            if self._event is None:
                host = {k: (None if v is None else v.clone()) for k, v in self._bufs.items()}
            else:
                side = torch.cuda.Stream(self._tr.flat_p.device)
                side.wait_event(self._event)
                with torch.cuda.stream(side):
                    host = {k: (None if v is None else torch.empty(v.shape, dtype=v.dtype, pin_memory=True).copy_(v, non_blocking=True))
                            for k, v in self._bufs.items()}
                side.synchronize()
            self._sd = self._tr._pack_state(host, self._scalars, self._qrows)
            self._bufs = {}
        return self._sd
