import contextlib
import os
import sys
import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(name):
    """Returns (params, grads, inputs, input_grads, outs, cots) of a module_case fixture."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    t = lambda k: torch.from_numpy(z[k])
    pick = lambda pre: {k[len(pre):]: t(k) for k in z.files if k.startswith(pre)}
    outs = [t(f"out{i}") for i in range(16) if f"out{i}" in z.files]
    cots = [t(f"cot{i}") for i in range(16) if f"cot{i}" in z.files]
    return pick("p."), pick("g."), pick("in."), pick("gin."), outs, cots


def load_npz(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind in "fi" else z[k]) for k in z.files}


def rel_l2(a, b):
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def assert_close(a, b, tol, what="", atol=0.0):
    """rel-L2 check; `atol` (per-element RMS) absorbs tensors that are mathematically zero
    (e.g. the gradient of a bias that an InstanceNorm removes) and hold only round-off."""
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    err = float((a - b).norm())
    bound = tol * float(b.norm()) + atol * (b.numel() ** 0.5)
    assert err <= bound, f"{what}: |err| {err:.3e} > {bound:.3e} (rel-L2 {err / (float(b.norm()) + 1e-30):.3e}, tol {tol:.1e})"


def check_update_deltas(z, names, deltas, lr=1e-3):
    """The update itself, p_after - p_before, against the reference's.  The first AdamW step moves every element by
    -lr * g / (|g| + eps) - lr * wd * p: by ~lr in the direction of -sign(g), whatever |g| is.  So the MAGNITUDE of the update is
    checked everywhere (it catches a missing / doubled / mis-scaled update), and its SIGN wherever the gradient is well above the
    fp32 round-off of the reference itself (an element whose gradient is noise moves by +-lr at random on both sides):
      * 1-element tensors (the 360 scalar mixes) whose |g| >= 5e-4 of the total norm: the value of the update;
      * every tensor: the absolute sum (5 %), and the sum up to the flips of a few % of near-zero-gradient elements.
    (Gradient directions themselves are pinned by the grad_probe check; the AdamW arithmetic by tests/test_trainer_gpu.py.)"""
    small = iter(torch.split(z["delta_small"].double(), [int(n) for n in z["delta_small_sizes"]]))
    gn, gtot = z["grad_norms"].double(), float(z["grad_total_norm"])
    checked_scalars = 0
    for i, (k, d) in enumerate(zip(names, deltas)):
        n = d.numel()
        d = d.flatten().cpu()
        ref = next(small) if n <= 8 else None
        if float(gn[i]) < 0:
            assert float(d.abs().max()) == 0.0, f"{k}: a parameter without gradient must not move"
            continue
        # 5 %: a gradient that is ~eps = 1e-9 after clipping gives |g| / (|g| + eps) anywhere below 1, and its round-off moves that
        assert abs(float(d.abs().sum()) - float(z["delta_abs"][i])) <= 0.05 * lr * n + 1e-12, f"{k}: |update| sum {float(d.abs().sum())} vs {float(z['delta_abs'][i])}"
        if n == 1 and float(gn[i]) >= 5e-4 * gtot:
            checked_scalars += 1
            assert float((d - ref).abs().max()) <= 0.02 * lr, f"{k}: update {d.tolist()} vs reference {ref.tolist()}"
        elif n > 1:
            assert abs(float(d.sum()) - float(z["delta_sum"][i])) <= 3 * lr * n ** 0.5 + 0.05 * lr * n, f"{k}: update sum"
    assert checked_scalars >= 30, checked_scalars


def _e4m3_bytes(t):
    """e4m3 bytes of an fp32 tensor (saturating), as the kernels write them"""
    return t.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


# ------------------------------------------------------------------------------------------- column views of wider buffers
# A quiet NaN with a recognisable payload, per element width: arithmetic produces the canonical NaN (payload 0), never this one, so
# "the kernel left this element alone" is an exact comparison of bits — through an integer view, for fp32 and bf16 alike.
_POISON_BITS = {torch.float32: (torch.int32, 0x7FC5A5A5), torch.bfloat16: (torch.int16, 0x7FE5)}


def bits(t):
    """integer view of an fp32 / bf16 tensor (same shape, same memory)"""
    return t.view(_POISON_BITS[t.dtype][0])


def poison_bits(dtype):
    """the output poison of embed() as the integer bits() shows it"""
    return _POISON_BITS[dtype][1]


def embed(t, left, right, *, poison):
    """(M, C) tensor t -> (buf, view): buf a fresh (M, left + C + right) tensor of t's dtype and device, view = buf[:, left:left + C]
    holding t, every other column poisoned: poison="nan" for an input operand (a result may not depend on a neighbour in any way, not
    even multiplied by zero), poison="bits" for an output (the payload NaN above: assert_pads_untouched compares it bit for bit)."""
    assert t.dim() == 2 and poison in ("nan", "bits")
    M, C = t.shape
    buf = torch.empty((M, left + C + right), dtype=t.dtype, device=t.device)
    if poison == "nan":
        buf.fill_(float("nan"))
    else:
        bits(buf).fill_(_POISON_BITS[t.dtype][1])
    view = buf[:, left:left + C]
    view.copy_(t)
    return buf, view


def assert_pads_untouched(buf, left, C, what):
    """every column of buf outside [left, left + C) still holds the output poison of embed(); names the first touched (row, column)"""
    want = _POISON_BITS[buf.dtype][1]
    touched = bits(buf) != want
    touched[:, left:left + C] = False
    if bool(touched.any()):
        r, c = (int(v) for v in touched.nonzero()[0])
        raise AssertionError(f"{what}: pad element (row {r}, column {c}) of a {tuple(buf.shape)} buffer was written "
                             f"(payload columns {left}..{left + C - 1}, bits {int(bits(buf)[r, c]) & (0xFFFFFFFF if buf.dtype == torch.float32 else 0xFFFF):#x})")


# ------------------------------------------------------------------------------------------- guarded, poisoned workspaces
# The scratch workspaces (ops._ws) are memory the kernels write and nothing else looks at: an overrun of the queried size lands in the
# allocator's slack, a fold that reads a partial row nobody wrote finds last call's right numbers there.  Under guarded_workspaces every
# workspace is its own buffer [front guard | payload | rear guard] filled with the output poison above (a payload NaN as fp32, garbage as
# an arrival counter): an overrun changes a guard byte, an unwritten cell reaches the result as a NaN.
_WS_POISON = _POISON_BITS[torch.float32][1]
_WS_FRONT, _WS_PAGE, _WS_REAR_MAX = 4096, 4096, 1 << 20   # the front guard keeps the 256 / 512-byte alignment of a fresh allocation


class GuardedWorkspaces:
    def __init__(self):
        self.records = []   # (buffer, payload bytes, requested bytes, caller)

    @property
    def calls(self):
        return len(self.records)

    @staticmethod
    def rear_bytes(n):
        return min(_WS_REAR_MAX, (max(_WS_PAGE, int(n)) + _WS_PAGE - 1) // _WS_PAGE * _WS_PAGE)

    @staticmethod
    def _caller():
        f = sys._getframe(1)
        while f is not None and f.f_code.co_filename == __file__:
            f = f.f_back
        if f is None:
            return "?"
        fn, self_ = f.f_code.co_name, f.f_locals.get("ctx", None)
        cls = type(self_).__name__.replace("Backward", "") if self_ is not None and fn in ("forward", "backward") else ""
        return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} {cls + '.' if cls else ''}{fn}"

    def alloc(self, n, device, caller=None):
        """`n` bytes (at least 16, as ops._ws hands out) of poisoned workspace between two poisoned guards"""
        n = int(n)
        pay = max(n, 16)
        total = (_WS_FRONT + pay + self.rear_bytes(n) + 3) // 4 * 4
        buf = torch.empty(total, dtype=torch.uint8, device=device)
        buf.view(torch.int32).fill_(_WS_POISON)
        self.records.append((buf, pay, n, caller or self._caller()))
        return buf[_WS_FRONT:_WS_FRONT + pay]

    def check(self):
        """every guard byte of every workspace handed out still holds the poison"""
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        for buf, pay, n, caller in self.records:
            want = torch.tensor([_WS_POISON], dtype=torch.int32, device=buf.device).view(torch.uint8).repeat(buf.numel() // 4)
            touched = buf != want
            touched[_WS_FRONT:_WS_FRONT + pay] = False
            if bool(touched.any()):
                at = int(touched.nonzero()[0])
                off = at - (_WS_FRONT + pay)
                raise AssertionError(f"workspace of {n} bytes taken by {caller}: guard byte at offset {off} from the end of the payload was written "
                                     f"({'front guard' if off < 0 else 'rear guard'}, {int(touched.sum())} guard bytes touched in all)")


@contextlib.contextmanager
def guarded_workspaces(monkeypatch):
    """with guarded_workspaces(monkeypatch) as g: every ops._ws inside is g.alloc; g.check() asserts the guards, g.calls counts the
    workspaces handed out, g.alloc(n, device) serves a test that calls the C ABI itself.  Works on CPU tensors too."""
    from adnm_hip import ops
    g = GuardedWorkspaces()
    with monkeypatch.context() as m:
        m.setattr(ops, "_ws", lambda nbytes, device: g.alloc(nbytes, device))
        yield g


# ------------------------------------------------------------------------------------------- poisoned outputs
# Outputs, saved statistics, intermediates and fresh gradient buffers come from torch.empty / torch.empty_like: a kernel whose grid, tail
# or early exit skips an element returns whatever the caching allocator handed back — usually the same op's right numbers of a moment ago.
# Under poisoned_outputs every such tensor arrives filled with a bit pattern.  Two patterns, because an integer or byte output may
# legitimately hold either value: an element that shows pattern 0 in run 0 AND pattern 1 in run 1 at the same index was written by nobody.
_OUT_NAN = {torch.float32: (torch.int32, (0x7FC5A5A5, 0x7FC3C3C3)), torch.bfloat16: (torch.int16, (0x7FE5, 0x7FD3)),
            torch.float16: (torch.int16, (0x7E5A, 0x7EA5)), torch.float64: (torch.int64, (0x7FF8A5A5A5A5A5A5, 0x7FF8C3C3C3C3C3C3))}
_OUT_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
assert _OUT_NAN[torch.float32][1][0] == _POISON_BITS[torch.float32][1] and _OUT_NAN[torch.bfloat16][1][0] == _POISON_BITS[torch.bfloat16][1]
WORKSPACE = "workspace"   # the role of an allocation made through ops._ws (tests/test_workspace_contract_gpu.py owns those)


def output_pattern(dtype, pattern):
    """-> (integer view dtype, the pattern as that signed integer): a payload NaN for floating types, 0x5A.. / 0xA5.. bytes for the rest"""
    if dtype in _OUT_NAN:
        view, pats = _OUT_NAN[dtype]
        return view, pats[pattern]
    size = torch.empty((), dtype=dtype).element_size()   # integers, bool, bytes, fp8
    v = int.from_bytes(bytes([(0x5A, 0xA5)[pattern]]) * size, "little", signed=True)
    return _OUT_INT[size], v


def pattern_mask(t, pattern):
    """bool tensor of t's shape: the elements that hold output pattern `pattern`, bit for bit"""
    view, v = output_pattern(t.dtype, pattern)
    return t.view(view) == v


class PoisonedOutputs:
    """stands in for the `torch` of a module: every attribute is torch's, except empty / empty_like, which fill what they return"""

    def __init__(self, pattern):
        assert pattern in (0, 1)
        self.pattern = pattern
        self.records = []   # (tensor, site, role, file:line)

    def __getattr__(self, name):
        return getattr(torch, name)

    def _site(self):
        """(site, role, where) of the caller outside this file, as GuardedWorkspaces._caller finds it; the role is the target the
        source line assigns to (`mu` of `mu = torch.empty(...)`), WORKSPACE for ops._ws"""
        import linecache
        f = sys._getframe(1)
        while f is not None and f.f_code.co_filename == __file__:
            f = f.f_back
        if f is None:
            return "?", "", "?"
        fn, base = f.f_code.co_name, os.path.basename(f.f_code.co_filename)
        if fn == "_ws" and base == "ops.py":
            site, _, where = self._outer(f.f_back)
            return site, WORKSPACE, where
        return self._outer(f, linecache)

    @staticmethod
    def _outer(f, linecache=None):
        if f is None:
            return "?", "", "?"
        fn, base, self_ = f.f_code.co_name, os.path.basename(f.f_code.co_filename), f.f_locals.get("ctx", None)
        cls = type(self_).__name__.replace("Backward", "") if self_ is not None and fn in ("forward", "backward") else ""
        role = ""
        if linecache is not None:
            line = linecache.getline(f.f_code.co_filename, f.f_lineno)
            head = line.split("torch.empty")[0]
            role = head.rsplit("=", 1)[0].strip() if "=" in head else ""
        return f"{base} {cls + '.' if cls else ''}{fn}", role, f"{base}:{f.f_lineno}"

    def _fill(self, t):
        if t.device.type == "meta":
            return t
        if t.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("poisoned_outputs: allocation under stream capture (the fill would become a graph node)")
        view, v = output_pattern(t.dtype, self.pattern)
        if t.numel():
            t.view(view).fill_(v)
        self.records.append((t,) + self._site())
        return t

    def empty(self, *args, **kwargs):
        return self._fill(torch.empty(*args, **kwargs))

    def empty_like(self, *args, **kwargs):
        return self._fill(torch.empty_like(*args, **kwargs))


POISONED_MODULES = ("adnm_hip.ops", "adnm_hip.validate", "adnm_hip.forecast", "adnm_hip.dataio", "adnm_hip.evaluator", "models.ADNssd", "models.Vssd")


@contextlib.contextmanager
def poisoned_outputs(monkeypatch, pattern):
    """with poisoned_outputs(monkeypatch, 0) as p: torch.empty / torch.empty_like of the POISONED_MODULES return tensors filled with output
    pattern 0 (or 1); p.records lists (tensor, site, role, file:line) per allocation.  Production code is not changed: the modules see a
    proxy as their `torch` for the length of the context.  Works on CPU tensors too."""
    import importlib
    p = PoisonedOutputs(pattern)
    with monkeypatch.context() as m:
        for name in POISONED_MODULES:
            m.setattr(importlib.import_module(name), "torch", p)
        yield p


def unwritten(rec0, rec1):
    """{(site, role): (elements, file:line, first flat index)} over the allocation sites of two runs of the same code, one per pattern:
    the elements that still hold pattern 0 in run 0 and pattern 1 in run 1 at the same index.  Workspaces are skipped."""
    assert [(r[1], r[2], tuple(r[0].shape), r[0].dtype) for r in rec0] == [(r[1], r[2], tuple(r[0].shape), r[0].dtype) for r in rec1], \
        "the two runs did not allocate the same tensors in the same order"
    found = {}
    for (t0, site, role, where), (t1, _, _, _) in zip(rec0, rec1):
        if role == WORKSPACE or t0.numel() == 0:
            continue
        both = pattern_mask(t0, 0) & pattern_mask(t1, 1)
        n = int(both.sum())
        if n:
            first = int(both.flatten().nonzero()[0])
            old = found.get((site, role))
            found[(site, role)] = (n + (old[0] if old else 0), old[1] if old else where, old[2] if old else first)
    return found
