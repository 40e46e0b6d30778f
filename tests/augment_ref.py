"""The CPU yardstick of the augmenting fetch (include/adnm_hip.h: adnm_batch_fetch_aug), written with torch's own slicing,
flip and transpose and nothing of the kernel's index arithmetic.  Comparisons go through the bit patterns, so that NaN payloads, -0.0
and infinities count."""
import torch


def decode(word):
    """-> (flip_lr, flip_ud, transpose, oy, ox, bit31) of one word, read off the table in the header (not through dataio.unpack_word)"""
    w = int(word) & 0xFFFFFFFF
    return bool(w & 1), bool(w & 2), bool(w & 4), (w >> 3) & 0x3FFF, (w >> 17) & 0x3FFF, bool(w >> 31)


def served(sample, word, H, W):
    """sample: (T, Hs, Ws) -> the (T, H, W) frames the word asks for, or None where the kernel must answer with NaNs"""
    flip_lr, flip_ud, transpose, oy, ox, bit31 = decode(word)
    T, Hs, Ws = sample.shape
    if bit31 or oy + H > Hs or ox + W > Ws or (transpose and H != W):
        return None
    w = sample[:, oy:oy + H, ox:ox + W]
    if flip_ud:
        w = w.flip(-2)
    if flip_lr:
        w = w.flip(-1)
    if transpose:
        w = w.transpose(-1, -2)
    return w.contiguous()


def batch(store, order, words, pos, B, t_in, H, W):
    """-> (x (B, t_in, H, W), tgt (B, T - t_in, H, W), the samples that must be all NaN) for positions pos .. pos + B of the epoch"""
    n, T = store.shape[:2]
    x, tgt, bad = torch.zeros(B, t_in, H, W), torch.zeros(B, T - t_in, H, W), []
    for b in range(B):
        s, w = int(order[pos + b]), None
        if 0 <= s < n:
            w = served(store[s], int(words[pos + b]), H, W)
        if w is None:
            bad.append(b)
            x[b], tgt[b] = float("nan"), float("nan")
        else:
            x[b], tgt[b] = w[:t_in], w[t_in:]
    return x, tgt, bad


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
