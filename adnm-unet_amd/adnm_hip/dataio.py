"""The input side of the hot path: datasets/Shanghai.py:52-59,121 turns every uint8 radar sample
(25, H0, W0) into float32, divides by 255, resizes to (S, S) with torchvision's tensor Resize (bilinear, align_corners=False, no
antialias) on the CPU, and train.py:133-134 copies the float batch to the GPU from pageable memory, synchronously.

RadarIngest moves the BYTES instead (4x less PCIe traffic than floats, and before the resize: the source frames are larger than
the model's input): two pinned host staging buffers and two device byte buffers alternate, the copy of batch i+1 runs on its own
stream beside the compute of batch i, and one HIP kernel (csrc/dataio.hip::radar_ingest) does / 255 + resize + the
(B, T, 1, S, S) layout on the device."""
import numpy as np
import torch

from . import lib


class RadarIngest:
    def __init__(self, batch, frames, H0, W0, size, device, in_frames=5):
        self.shape = (batch, frames, H0, W0)
        self.size, self.in_frames, self.device = size, in_frames, torch.device(device)
        self.pinned = [torch.empty(self.shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev = [torch.empty(self.shape, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.ready = [torch.cuda.Event() for _ in range(2)]
        self.consumed = [torch.cuda.Event() for _ in range(2)]
        self._slot = 0
        self._pending = []            # FIFO of submitted, not yet taken slots (prefetch depth <= 2 = the number of slots)

    def submit(self, batch_u8):
        """Start moving a (B, T, H0, W0) uint8 batch (numpy array or CPU tensor) to the device; returns at once.
        At most two batches may be in flight (one per slot): a third submit() without a take() raises instead of overwriting a
        staging buffer whose host-to-device copy may still be running."""
        if len(self._pending) >= 2:
            raise RuntimeError("RadarIngest.submit(): both staging slots hold batches that were never taken (prefetch depth is 2)")
        s = self._slot
        self._slot ^= 1
        src = torch.from_numpy(batch_u8) if isinstance(batch_u8, np.ndarray) else batch_u8
        if tuple(src.shape) != self.shape or src.dtype != torch.uint8:
            raise RuntimeError(f"RadarIngest: expected uint8 {self.shape}, got {src.dtype} {tuple(src.shape)}")
        self.consumed[s].synchronize()          # the kernel that read this slot's previous contents has finished
        self.pinned[s].copy_(src)               # host memcpy into pinned memory
        with torch.cuda.stream(self.copy_stream):
            self.dev[s].copy_(self.pinned[s], non_blocking=True)
            self.ready[s].record(self.copy_stream)
        self._pending.append(s)

    def take(self):
        """-> (imgs (B, T_in, 1, S, S), targets (B, T_out, 1, S, S)) fp32 on the device, as train.py:133 splits them."""
        if not self._pending:
            raise RuntimeError("RadarIngest.take() without a submitted batch")
        s = self._pending.pop(0)
        B, T, H0, W0 = self.shape
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self.ready[s])
        out = torch.empty((B, T, 1, self.size, self.size), dtype=torch.float32, device=self.device)
        lib.call("adnm_radar_ingest", self.dev[s].data_ptr(), out.data_ptr(), B * T, H0, W0, self.size, 1.0 / 255.0, cur.cuda_stream)
        self.consumed[s].record(cur)
        return out[:, :self.in_frames], out[:, self.in_frames:]


def ingest(batch_u8_device, size):
    """One-shot form on bytes already resident on the device: (B, T, H0, W0) uint8 -> (B, T, 1, S, S) fp32."""
    B, T, H0, W0 = batch_u8_device.shape
    if not batch_u8_device.is_cuda or batch_u8_device.dtype != torch.uint8:
        raise RuntimeError("ingest: needs a uint8 GPU tensor")
    src = batch_u8_device.contiguous()
    out = torch.empty((B, T, 1, size, size), dtype=torch.float32, device=src.device)
    lib.call("adnm_radar_ingest", src.data_ptr(), out.data_ptr(), B * T, H0, W0, size, 1.0 / 255.0, torch.cuda.current_stream().cuda_stream)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# The resident split.  The reference builds every sample of a split once at import (datasets/Shanghai.py:121-136) and
# hands the list to DataLoader(shuffle=True, drop_last=True), which collates and copies a batch per step (train.py:44-57,132-134).
# Here the split is ingested once and stays on the device; per step ONE kernel (csrc/dataio.hip::batch_fetch) writes the next batch
# into the buffers the trainer's or the validator's graph reads, in the DataLoader's own order.
class EpochOrder:
    """The sampler of DataLoader(dataset, batch, shuffle, drop_last=True, generator=generator), restated on the host (no GPU needed).

    next_epoch() -> the epoch's index vector (int32, length n), made with the draws the loader makes on the same generator: the
    iterator's base seed (one int64 .random_()), then, shuffled, RandomSampler's randperm(n) and the randperm(n) it draws for the
    remainder (drawn even when the remainder is empty); with generator=None the base seed and a sampler seed come from the default
    generator and the permutation from a fresh generator seeded with the latter.  next_batch() -> this rank's indices of the next step:
    global batch g is perm[g*B*W : (g+1)*B*W] and rank r takes its r-th contiguous chunk (nn.DataParallel's scatter, train.py:99-102).
    drop_last=True is the only mode (all three loaders of the reference use it): steps = n // (batch * world)."""

    def __init__(self, n, batch, shuffle=True, generator=None, rank=0, world=1):
        n, batch, rank, world = int(n), int(batch), int(rank), int(world)
        if batch < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"EpochOrder: batch {batch}, rank {rank} of {world}")
        if not 0 < n < 2 ** 31:
            raise ValueError(f"EpochOrder: {n} samples (1 .. 2^31 - 1: the indices are int32)")
        if n < batch * world:
            raise ValueError(f"EpochOrder: {n} samples give no full batch of {batch} x {world} ranks (drop_last=True)")
        self.n, self.batch, self.shuffle, self.generator, self.rank, self.world = n, batch, bool(shuffle), generator, rank, world
        self.steps = n // (batch * world)
        self.epoch = 0       # epochs begun
        self.pos = 0         # steps taken in the current one
        self.perm = None

    def __len__(self):
        return self.steps

    def next_epoch(self):
        g = self.generator
        torch.empty((), dtype=torch.int64).random_(generator=g)          # _BaseDataLoaderIter's base seed
        if not self.shuffle:
            perm = torch.arange(self.n)
        elif g is None:
            fresh = torch.Generator()
            fresh.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
            perm = torch.randperm(self.n, generator=fresh)
        else:
            perm = torch.randperm(self.n, generator=g)
            torch.randperm(self.n, generator=g)                          # RandomSampler's remainder draw: made, then sliced to nothing
        self.perm = perm.to(torch.int32)
        self.epoch += 1
        self.pos = 0
        return self.perm

    def offset(self, step=None):
        """-> where this rank's batch of `step` (default: the next one) starts in the epoch's index vector"""
        step = self.pos if step is None else int(step)
        if self.perm is None:
            raise RuntimeError("EpochOrder: no epoch yet (next_epoch() first)")
        if not 0 <= step < self.steps:
            raise IndexError(f"EpochOrder: step {step} of an epoch of {self.steps} steps (next_epoch() starts the next one)")
        return (step * self.world + self.rank) * self.batch

    def next_batch(self):
        """-> this rank's indices of the next step; the position moves on.  Past the end of the epoch: IndexError."""
        o = self.offset()
        self.pos += 1
        return self.perm[o:o + self.batch]

    def state_dict(self):
        """Python scalars and tensors: fits checkpoint.save_training_state's schedule_stats beside ReferenceSelection's.  "generator" is
        the generator's state; with generator=None it is the DEFAULT generator's, which load_state_dict() puts back as well (the next
        epoch's order comes from it)."""
        g = self.generator
        return {"n": self.n, "batch": self.batch, "world": self.world, "shuffle": self.shuffle, "epoch": self.epoch, "pos": self.pos,
                "perm": None if self.perm is None else self.perm.clone(),
                "generator": (torch.get_rng_state() if g is None else g.get_state()).clone()}

    def load_state_dict(self, sd):
        for k in ("n", "batch", "world", "shuffle"):
            if sd[k] != getattr(self, k):
                raise ValueError(f"EpochOrder.load_state_dict: saved with {k} = {sd[k]}, this order has {getattr(self, k)}")
        perm = sd["perm"]
        if perm is not None and (perm.dtype != torch.int32 or tuple(perm.shape) != (self.n,)):
            raise ValueError(f"EpochOrder.load_state_dict: the permutation is {perm.dtype} {tuple(perm.shape)}, expected int32 ({self.n},)")
        if not 0 <= int(sd["pos"]) <= self.steps:
            raise ValueError(f"EpochOrder.load_state_dict: position {sd['pos']} in an epoch of {self.steps} steps")
        state = sd["generator"].to("cpu", torch.uint8)
        if self.generator is None:
            torch.set_rng_state(state)
        else:
            self.generator.set_state(state)
        self.epoch, self.pos = int(sd["epoch"]), int(sd["pos"])
        self.perm = None if perm is None else perm.to("cpu").clone()


class ResidentDataset:
    """A whole split on the device and its batches by kernel.

        feed = ResidentDataset.from_bytes(frames_u8, size=128, in_frames=5, batch=4, device="cuda", generator=g)
        for epoch in ...:
            feed.begin_epoch()                  # the epoch's order: 4*N bytes to the device, the one copy per epoch
            for _ in range(len(feed)):
                loss = trainer.step_from(feed)  # one launch in front of the graph replay, into the graph's static buffers

    store: (N, T, S, S) fp32; order: (N,) int32 on the device.  The position is a kernel ARGUMENT, kept on the host; the fetch runs on
    the current stream.  state_dict() is the order's: the store is not saved."""

    def __init__(self, store, in_frames, batch, shuffle=True, generator=None, rank=0, world=1):
        if not (torch.is_tensor(store) and store.is_cuda and store.dtype == torch.float32 and store.dim() == 4 and store.is_contiguous()):
            raise RuntimeError("ResidentDataset: the store is a contiguous fp32 (N, T, H, W) GPU tensor (from_bytes / from_frames build it)")
        N, T, H, W = store.shape
        if not 1 <= int(in_frames) < T:
            raise ValueError(f"ResidentDataset: in_frames {in_frames} of {T} frames per sample")
        self.store, self.in_frames, self.batch, self.device = store, int(in_frames), int(batch), store.device
        self.order = EpochOrder(N, batch, shuffle=shuffle, generator=generator, rank=rank, world=world)
        self._order_dev = torch.empty(N, dtype=torch.int32, device=store.device)
        self._order_pin = torch.empty(N, dtype=torch.int32).pin_memory()   # the upload is asynchronous: the host never waits for the stream
        self._order_sent = None      # the event behind the last upload (the pinned image may be rewritten once it has passed)
        self._uploaded = None        # the epoch whose order _order_dev holds

    @staticmethod
    def _alloc_store(shape, device):
        need = 4
        for d in shape:
            need *= int(d)
        try:
            return torch.empty(shape, dtype=torch.float32, device=device)
        except torch.OutOfMemoryError as e:
            raise RuntimeError(f"ResidentDataset: the store {tuple(shape)} fp32 needs {need} bytes of device memory, which did not fit ({e})") from None

    @classmethod
    def from_bytes(cls, frames_u8, size, in_frames, batch, device, shuffle=True, generator=None, rank=0, world=1, chunk=64):
        """frames_u8: (N, T, H0, W0) uint8, numpy or CPU tensor.  Moved in chunks of `chunk` samples through two pinned staging buffers
        and ingested with adnm_radar_ingest (/255 and the resize on the device): store[i] is bit for bit dataio.ingest(sample i, size)."""
        src = torch.from_numpy(frames_u8) if isinstance(frames_u8, np.ndarray) else frames_u8
        if not torch.is_tensor(src) or src.is_cuda or src.dtype != torch.uint8 or src.dim() != 4:
            raise RuntimeError("ResidentDataset.from_bytes: expected (N, T, H0, W0) uint8 in host memory")
        device, chunk = torch.device(device), max(1, min(int(chunk), src.shape[0]))
        N, T, H0, W0 = src.shape
        store = cls._alloc_store((N, T, size, size), device)
        pinned = [torch.empty((chunk, T, H0, W0), dtype=torch.uint8).pin_memory() for _ in range(2)]
        dev = [torch.empty((chunk, T, H0, W0), dtype=torch.uint8, device=device) for _ in range(2)]
        done = [None, None]
        with torch.cuda.device(device):
            cur = torch.cuda.current_stream()
            for k, lo in enumerate(range(0, N, chunk)):
                s, n = k & 1, min(chunk, N - lo)
                if done[s] is not None:
                    done[s].synchronize()                  # the copy out of this staging buffer has finished
                pinned[s][:n].copy_(src[lo:lo + n])
                dev[s][:n].copy_(pinned[s][:n], non_blocking=True)
                done[s] = torch.cuda.Event()
                done[s].record(cur)
                lib.call("adnm_radar_ingest", dev[s].data_ptr(), store[lo:lo + n].data_ptr(), n * T, H0, W0, size, 1.0 / 255.0, cur.cuda_stream)
            cur.synchronize()
        del pinned, dev                                    # staging is given back; the store stays
        return cls(store, in_frames, batch, shuffle=shuffle, generator=generator, rank=rank, world=world)

    @classmethod
    def from_frames(cls, frames_f32, in_frames, batch, device, shuffle=True, generator=None, rank=0, world=1):
        """frames_f32: (N, T, H, W) or (N, T, 1, H, W) float32 that is final (the LAPS fields): kept bit for bit, no resize."""
        src = torch.from_numpy(frames_f32) if isinstance(frames_f32, np.ndarray) else frames_f32
        if torch.is_tensor(src) and src.dim() == 5 and src.shape[2] == 1:
            src = src[:, :, 0]
        if not torch.is_tensor(src) or src.dtype != torch.float32 or src.dim() != 4:
            raise RuntimeError("ResidentDataset.from_frames: expected (N, T, H, W) float32")
        store = cls._alloc_store(tuple(src.shape), torch.device(device))
        store.copy_(src)
        return cls(store, in_frames, batch, shuffle=shuffle, generator=generator, rank=rank, world=world)

    # ---- shapes
    @property
    def x_shape(self):
        N, T, H, W = self.store.shape
        return (self.batch, self.in_frames, 1, H, W)

    @property
    def tgt_shape(self):
        N, T, H, W = self.store.shape
        return (self.batch, T - self.in_frames, 1, H, W)

    def __len__(self):
        return self.order.steps

    @property
    def store_bytes(self):
        return self.store.numel() * 4

    # ---- per epoch, per step
    def _upload(self):
        """the epoch's order to the device, on the current stream (behind the last fetch of the epoch before, which read the old one)"""
        if self._order_sent is not None:
            self._order_sent.synchronize()
        self._order_pin.copy_(self.order.perm)
        self._order_dev.copy_(self._order_pin, non_blocking=True)
        self._order_sent = torch.cuda.Event()
        self._order_sent.record(torch.cuda.current_stream(self.device))
        self._uploaded = self.order.epoch

    def begin_epoch(self):
        self.order.next_epoch()
        self._upload()

    def _check(self, t, shape, what):
        if not (torch.is_tensor(t) and t.device == self.device and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"ResidentDataset.fetch_into: {what} must be a contiguous fp32 tensor on {self.device}")
        N, T, H, W = self.store.shape
        if t.numel() != shape[0] * shape[1] * H * W or t.shape[0] != shape[0] or t.shape[1] != shape[1] or tuple(t.shape[-2:]) != (H, W):
            raise RuntimeError(f"ResidentDataset.fetch_into: {what} is {tuple(t.shape)}, the feed gives {shape} (or the same without the channel axis)")

    def fetch_into(self, x, tgt):
        """The next batch into x (B, T_in, 1, S, S) and tgt (B, T_out, 1, S, S) (the channel axis may be missing): one launch on the
        current stream of the store's device (which must be the current device, as for every entry point).  Past the end of the epoch:
        IndexError (begin_epoch() starts the next)."""
        self._check(x, self.x_shape, "x")
        self._check(tgt, self.tgt_shape, "tgt")
        self._launch(x, tgt)

    def _launch(self, x, tgt):
        """fetch_into() on destinations the caller has checked once (a trainer's static buffers: the per-step host path stays short)"""
        order = self.order
        if order.perm is None:
            raise RuntimeError("ResidentDataset: no epoch yet (begin_epoch() first)")
        if self._uploaded != order.epoch:           # a restored order: its permutation goes to the device before the first fetch
            self._upload()
        N, T, H, W = self.store.shape
        lib.call("adnm_batch_fetch", self.store.data_ptr(), N, T, H * W, self._order_dev.data_ptr(), N, order.offset(), x.data_ptr(), tgt.data_ptr(),
                 self.batch, self.in_frames, torch.cuda.current_stream(self.device).cuda_stream)
        order.pos += 1

    def fetch(self):
        x = torch.empty(self.x_shape, dtype=torch.float32, device=self.device)
        tgt = torch.empty(self.tgt_shape, dtype=torch.float32, device=self.device)
        self.fetch_into(x, tgt)
        return x, tgt

    def state_dict(self):
        return self.order.state_dict()

    def load_state_dict(self, sd):
        self.order.load_state_dict(sd)
        self._uploaded = None
