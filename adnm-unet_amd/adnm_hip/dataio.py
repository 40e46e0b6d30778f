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


# ---------------------------------------------------------------------------------------------------------------------------------
# Augmentation in the fetch.  The reference has none (its only transform is the resize, datasets/Shanghai.py:40-59).
# One int32 word per POSITION of the epoch tells csrc/dataio.hip::batch_fetch_aug which window of the stored frame to serve and under
# which of the square's eight symmetries.  pack_word / unpack_word are the one statement of the layout on the host
# (include/adnm_hip.h: adnm_batch_fetch_aug is the one on the device side).
FLIP_H, FLIP_V, TRANSPOSE = 1, 2, 4      # bit 0: flip left-right, bit 1: flip up-down, bit 2: transpose
OFFSET_LIMIT = 1 << 14                   # oy (bits 3-16) and ox (bits 17-30) are 14-bit fields; bit 31 stays 0


def pack_word(code, oy, ox):
    """(code in 0..7, oy, ox in 0..16383) -> the word; Python ints give an int, tensors an int32 tensor"""
    if torch.is_tensor(code) or torch.is_tensor(oy) or torch.is_tensor(ox):
        code, oy, ox = (torch.as_tensor(v).to(torch.int64) for v in (code, oy, ox))
        if bool(((code < 0) | (code > 7) | (oy < 0) | (oy >= OFFSET_LIMIT) | (ox < 0) | (ox >= OFFSET_LIMIT)).any()):
            raise ValueError("pack_word: a code outside 0..7 or an offset outside 0..16383")
        return (code | (oy << 3) | (ox << 17)).to(torch.int32)
    code, oy, ox = int(code), int(oy), int(ox)
    if not (0 <= code <= 7 and 0 <= oy < OFFSET_LIMIT and 0 <= ox < OFFSET_LIMIT):
        raise ValueError(f"pack_word: code {code} (0..7), oy {oy}, ox {ox} (0..16383)")
    return code | (oy << 3) | (ox << 17)


def unpack_word(word):
    """-> (code, oy, ox), ints for an int and int64 tensors for a tensor"""
    w = word.to(torch.int64) if torch.is_tensor(word) else int(word)
    return w & 7, (w >> 3) & (OFFSET_LIMIT - 1), (w >> 17) & (OFFSET_LIMIT - 1)


class Augment:
    """Which augmentations a feed draws, and the generator it draws them from.

    The generator is PRIVATE and seeded with `seed`: nothing is ever drawn from the default generator or from the EpochOrder's, so the
    order stays the DataLoader's, batch for batch.  draw() always makes its draws in this order: randint(0, 8, (n,)) & mask, then
    randint(0, span_y + 1, (n,)), then randint(0, span_x + 1, (n,)); with shift=False both offsets are the centre (span // 2) and
    nothing is drawn for them.  That fixed sequence is what makes a run reproducible from `seed` alone."""

    def __init__(self, flip_h=True, flip_v=True, transpose=True, shift=True, seed=0):
        self.flip_h, self.flip_v, self.transpose, self.shift, self.seed = bool(flip_h), bool(flip_v), bool(transpose), bool(shift), int(seed)
        self.mask = (FLIP_H if self.flip_h else 0) | (FLIP_V if self.flip_v else 0) | (TRANSPOSE if self.transpose else 0)
        self.generator = torch.Generator()
        self.generator.manual_seed(self.seed)

    def spec(self):
        return {"flip_h": self.flip_h, "flip_v": self.flip_v, "transpose": self.transpose, "shift": self.shift, "seed": self.seed}

    def draw(self, n, span_y, span_x):
        """-> (n,) int32 words with offsets in [0, span_y] x [0, span_x] (span = stored side - served side)"""
        n, span_y, span_x = int(n), int(span_y), int(span_x)
        if not (0 <= span_y < OFFSET_LIMIT and 0 <= span_x < OFFSET_LIMIT):
            raise ValueError(f"Augment.draw: spans {span_y}, {span_x} outside 0..16383")
        code = torch.randint(0, 8, (n,), generator=self.generator) & self.mask
        if self.shift:
            oy = torch.randint(0, span_y + 1, (n,), generator=self.generator)
            ox = torch.randint(0, span_x + 1, (n,), generator=self.generator)
        else:
            oy, ox = torch.full((n,), span_y // 2), torch.full((n,), span_x // 2)
        return pack_word(code, oy, ox)


class EpochWords:
    """The words of an epoch beside an EpochOrder, on the host (no GPU needed): next_epoch() draws all n of them (every rank draws the
    same n from its identically seeded generator and reads its own positions, as it does for the order).  augment=None: the centre
    window, untransformed, every epoch (the validation feed of a cropped store); nothing is drawn and nothing is saved."""

    def __init__(self, n, span_y, span_x, augment=None):
        self.n, self.span_y, self.span_x, self.augment = int(n), int(span_y), int(span_x), augment
        if not (0 <= self.span_y < OFFSET_LIMIT and 0 <= self.span_x < OFFSET_LIMIT):
            raise ValueError(f"EpochWords: spans {span_y}, {span_x} outside 0..16383")
        self.words = None if augment is not None else torch.full((self.n,), pack_word(0, self.span_y // 2, self.span_x // 2), dtype=torch.int32)

    def next_epoch(self):
        if self.augment is not None:
            self.words = self.augment.draw(self.n, self.span_y, self.span_x)
        return self.words

    def _spec(self):
        return dict(self.augment.spec(), n=self.n, span_y=self.span_y, span_x=self.span_x)

    def state_into(self, sd):
        """adds the key "augment" (spec, the epoch's words, the generator's state) to a feed's state; without an Augment: nothing"""
        if self.augment is not None:
            sd["augment"] = {"spec": self._spec(), "words": None if self.words is None else self.words.clone(),
                             "generator": self.augment.generator.get_state().clone()}
        return sd

    def load_from(self, sd):
        if self.augment is None:
            if "augment" in sd:
                raise ValueError("ResidentDataset.load_state_dict: the state was saved by an augmenting feed, this feed has no Augment")
            return
        if "augment" not in sd:
            raise ValueError('ResidentDataset.load_state_dict: the state has no "augment" key (it was saved by a feed without augmentation), '
                             "this feed augments: its words and generator cannot be restored")
        st = sd["augment"]
        if st["spec"] != self._spec():
            raise ValueError(f"ResidentDataset.load_state_dict: saved with augmentation {st['spec']}, this feed has {self._spec()}")
        words = st["words"]
        if words is not None and (words.dtype != torch.int32 or tuple(words.shape) != (self.n,)):
            raise ValueError(f"ResidentDataset.load_state_dict: the words are {words.dtype} {tuple(words.shape)}, expected int32 ({self.n},)")
        self.augment.generator.set_state(st["generator"].to("cpu", torch.uint8))
        self.words = None if words is None else words.to("cpu").clone()


class ResidentDataset:
    """A whole split on the device and its batches by kernel.

        feed = ResidentDataset.from_bytes(frames_u8, size=128, in_frames=5, batch=4, device="cuda", generator=g)
        for epoch in ...:
            feed.begin_epoch()                  # the epoch's order: 4*N bytes to the device, the one copy per epoch
            for _ in range(len(feed)):
                loss = trainer.step_from(feed)  # one launch in front of the graph replay, into the graph's static buffers

    store: (N, T, S, S) fp32; order: (N,) int32 on the device.  The position is a kernel ARGUMENT, kept on the host; the fetch runs on
    the current stream.  state_dict() is the order's: the store is not saved.

    crop=(H, W) serves H x W windows of a larger stored frame, augment=Augment(...) flips, transposes and shifts them, in the fetch
    itself (adnm_batch_fetch_aug): begin_epoch() draws one word per position after the order and uploads both.
    from_bytes(size=160, crop=(128, 128)) keeps 160 x 160 and feeds 128 x 128: 1.56 times the store of size=128.  crop without augment
    (or with shift=False) is the centre window ((Hs - H) // 2, (Ws - W) // 2): the validation feed of a cropped store.  With neither
    argument nothing is allocated, adnm_batch_fetch is launched and state_dict() is the order's, as before; with an Augment it gains
    the key "augment" (the spec, the epoch's words, the generator's state)."""

    def __init__(self, store, in_frames, batch, shuffle=True, generator=None, rank=0, world=1, crop=None, augment=None):
        if not (torch.is_tensor(store) and store.is_cuda and store.dtype == torch.float32 and store.dim() == 4 and store.is_contiguous()):
            raise RuntimeError("ResidentDataset: the store is a contiguous fp32 (N, T, H, W) GPU tensor (from_bytes / from_frames build it)")
        N, T, H, W = store.shape
        if not 1 <= int(in_frames) < T:
            raise ValueError(f"ResidentDataset: in_frames {in_frames} of {T} frames per sample")
        self.served = self._served(H, W, crop, augment)
        self.store, self.in_frames, self.batch, self.device = store, int(in_frames), int(batch), store.device
        self.order = EpochOrder(N, batch, shuffle=shuffle, generator=generator, rank=rank, world=world)
        self._order_dev = torch.empty(N, dtype=torch.int32, device=store.device)
        self._order_pin = torch.empty(N, dtype=torch.int32, pin_memory=True)   # the upload is asynchronous: the host never waits for the stream
        self._order_sent = None      # the event behind the last upload (the pinned image may be rewritten once it has passed)
        self._uploaded = None        # the epoch whose order _order_dev holds
        self.augment, self.words = augment, None
        if crop is not None or augment is not None:
            self.words = EpochWords(N, H - self.served[0], W - self.served[1], augment)
            self._words_dev = torch.empty(N, dtype=torch.int32, device=store.device)
            self._words_pin = torch.empty(N, dtype=torch.int32, pin_memory=True)

    @staticmethod
    def _served(Hs, Ws, crop, augment):
        """-> the served frame (H, W); refuses what adnm_batch_fetch_aug would refuse or answer with NaNs"""
        if augment is not None and not isinstance(augment, Augment):
            raise TypeError("ResidentDataset: augment is an adnm_hip.dataio.Augment or None")
        H, W = (Hs, Ws) if crop is None else (int(crop[0]), int(crop[1]))
        if not (1 <= H <= Hs and 1 <= W <= Ws):
            raise ValueError(f"ResidentDataset: crop {(H, W)} of a stored frame of {(Hs, Ws)}")
        if (crop is not None or augment is not None) and not (Hs < OFFSET_LIMIT and Ws < OFFSET_LIMIT):
            raise ValueError(f"ResidentDataset: crop / augment need stored sides below {OFFSET_LIMIT}, the store has {(Hs, Ws)}")
        if augment is not None and augment.transpose and H != W:
            raise ValueError(f"ResidentDataset: transpose=True needs a square served frame, got {(H, W)}")
        return (H, W)

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
    def from_bytes(cls, frames_u8, size, in_frames, batch, device, shuffle=True, generator=None, rank=0, world=1, chunk=64, crop=None, augment=None):
        """frames_u8: (N, T, H0, W0) uint8, numpy or CPU tensor.  Moved in chunks of `chunk` samples through two pinned staging buffers
        and ingested with adnm_radar_ingest (/255 and the resize on the device): store[i] is bit for bit dataio.ingest(sample i, size).
        crop, augment: as in the constructor (the store is size x size, the feed serves crop)."""
        src = torch.from_numpy(frames_u8) if isinstance(frames_u8, np.ndarray) else frames_u8
        if not torch.is_tensor(src) or src.is_cuda or src.dtype != torch.uint8 or src.dim() != 4:
            raise RuntimeError("ResidentDataset.from_bytes: expected (N, T, H0, W0) uint8 in host memory")
        device, chunk = torch.device(device), max(1, min(int(chunk), src.shape[0]))
        N, T, H0, W0 = src.shape
        cls._served(size, size, crop, augment)             # a bad crop is refused before the split is moved
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
        return cls(store, in_frames, batch, shuffle=shuffle, generator=generator, rank=rank, world=world, crop=crop, augment=augment)

    @classmethod
    def from_frames(cls, frames_f32, in_frames, batch, device, shuffle=True, generator=None, rank=0, world=1, crop=None, augment=None):
        """frames_f32: (N, T, H, W) or (N, T, 1, H, W) float32 that is final (the LAPS fields): kept bit for bit, no resize."""
        src = torch.from_numpy(frames_f32) if isinstance(frames_f32, np.ndarray) else frames_f32
        if torch.is_tensor(src) and src.dim() == 5 and src.shape[2] == 1:
            src = src[:, :, 0]
        if not torch.is_tensor(src) or src.dtype != torch.float32 or src.dim() != 4:
            raise RuntimeError("ResidentDataset.from_frames: expected (N, T, H, W) float32")
        cls._served(src.shape[2], src.shape[3], crop, augment)
        store = cls._alloc_store(tuple(src.shape), torch.device(device))
        store.copy_(src)
        return cls(store, in_frames, batch, shuffle=shuffle, generator=generator, rank=rank, world=world, crop=crop, augment=augment)

    # ---- shapes
    @property
    def x_shape(self):
        H, W = self.served
        return (self.batch, self.in_frames, 1, H, W)

    @property
    def tgt_shape(self):
        T, (H, W) = self.store.shape[1], self.served
        return (self.batch, T - self.in_frames, 1, H, W)

    def __len__(self):
        return self.order.steps

    @property
    def store_bytes(self):
        return self.store.numel() * 4

    # ---- per epoch, per step
    def _upload(self):
        """the epoch's order (and words) to the device, on the current stream (behind the last fetch of the epoch before, which read the
        old ones)"""
        if self._order_sent is not None:
            self._order_sent.synchronize()
        self._order_pin.copy_(self.order.perm)
        self._order_dev.copy_(self._order_pin, non_blocking=True)
        if self.words is not None:
            if self.words.words is None:
                raise RuntimeError("ResidentDataset: the restored state holds an order but no words")
            self._words_pin.copy_(self.words.words)
            self._words_dev.copy_(self._words_pin, non_blocking=True)
        self._order_sent = torch.cuda.Event()
        self._order_sent.record(torch.cuda.current_stream(self.device))
        self._uploaded = self.order.epoch

    def begin_epoch(self):
        self.order.next_epoch()
        if self.words is not None:
            self.words.next_epoch()          # after the order, from the Augment's own generator: the order's draws are untouched
        self._upload()

    def _check(self, t, shape, what):
        if not (torch.is_tensor(t) and t.device == self.device and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"ResidentDataset.fetch_into: {what} must be a contiguous fp32 tensor on {self.device}")
        H, W = self.served
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
        if self.words is None:
            lib.call("adnm_batch_fetch", self.store.data_ptr(), N, T, H * W, self._order_dev.data_ptr(), N, order.offset(), x.data_ptr(), tgt.data_ptr(),
                     self.batch, self.in_frames, torch.cuda.current_stream(self.device).cuda_stream)
        else:
            lib.call("adnm_batch_fetch_aug", self.store.data_ptr(), N, T, H, W, self._order_dev.data_ptr(), self._words_dev.data_ptr(), N, order.offset(),
                     x.data_ptr(), tgt.data_ptr(), self.batch, self.in_frames, self.served[0], self.served[1],
                     torch.cuda.current_stream(self.device).cuda_stream)
        order.pos += 1

    def fetch(self):
        x = torch.empty(self.x_shape, dtype=torch.float32, device=self.device)
        tgt = torch.empty(self.tgt_shape, dtype=torch.float32, device=self.device)
        self.fetch_into(x, tgt)
        return x, tgt

    def state_dict(self):
        sd = self.order.state_dict()
        return sd if self.words is None else self.words.state_into(sd)

    def load_state_dict(self, sd):
        (self.words or EpochWords(self.order.n, 0, 0)).load_from(sd)   # refuses before anything is changed
        self.order.load_state_dict(sd)
        self._uploaded = None
