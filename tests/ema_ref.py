"""The fp64 statement of adnm_ema_update that the EMA tests check against, and its error bound (no test in here)."""
import torch


def warmup_decay(decay, t):
    """min(decay, (1 + t) / (10 + t)) in fp64: the d of optimiser step t"""
    return min(float(decay), (1.0 + t) / (10.0 + t))


def assert_ema_step(got, ema_before, p, d, what):
    """got = fmaf(d, ema_before, w * p) with w = float32(1) - float32(d), element by element:
    |got - ref| <= 2^-23 (|d ema| + |w p|) + 2^-126 against ref = d ema + w p in fp64.  The product w p and the fma round once each, so
    the error is at most u |w p| + u |d ema + w p| with u = 2^-24; 2^-126 covers results in the subnormal range."""
    d32 = torch.tensor(d, dtype=torch.float32)
    assert float(d32) == d, f"{what}: d = {d!r} is no fp32 value"
    w32 = torch.tensor(1.0, dtype=torch.float32) - d32
    dev = got.device   # (on the GPU for the 72 M elements of a trainer's buffers)
    a = ema_before.detach().to(dev).double().flatten() * float(d32)
    b = p.detach().to(dev).double().flatten() * float(w32)
    err = (got.detach().double().flatten() - (a + b)).abs()
    bound = 2.0 ** -23 * (a.abs() + b.abs()) + 2.0 ** -126
    bad = err > bound
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: element {i}: |got - ref| = {float(err[i]):.3e} > {float(bound[i]):.3e} (d = {d!r}, "
                             f"{int(bad.sum())} of {bad.numel()} elements out of bound)")
