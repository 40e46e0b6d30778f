"""The entry points of the moving average of the weights at the C boundary, without a GPU: declared in include/adnm_hip.h, exported by
the library, additive (the ABI version stays), validating their arguments before any launch; and the trainer's keywords."""
import ctypes
import inspect

import pytest

from adnm_hip import lib

NEW = ("adnm_ema_update", "adnm_ema_swap")


def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
        assert protos[name][0] == "int" and protos[name][1][-1] == "adnm_stream_t"
    assert protos["adnm_ema_update"][1] == ["const float*", "float*", "int64_t", "const float*", "float", "int", "float*", "const void*",
                                            "adnm_stream_t"]
    assert protos["adnm_ema_swap"][1] == ["float*", "float*", "int64_t", "adnm_stream_t"]
    assert lib.load().adnm_abi_version() == 11


def test_arguments_are_checked_on_the_host():
    """fake addresses: every call is refused on entry, nothing is launched"""
    so = lib.load()
    A, B, S, I = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    upd = lambda p, e, n, s=S, d=0.9, i=I, st=None: so.adnm_ema_update(p, e, n, s, d, 1, i, st, None)
    assert upd(None, B, 4) == -1 and "null pointer" in lib.last_error()
    assert upd(A, None, 4) == -1 and "null pointer" in lib.last_error()
    assert upd(A, B, 4, s=None) == -1 and "null pointer" in lib.last_error()
    assert upd(A, B, 4, i=None) == -1 and "null pointer" in lib.last_error()
    assert upd(A, B, 0) == -1 and "multiple of 4" in lib.last_error()
    assert upd(A, B, 6) == -1 and "multiple of 4" in lib.last_error()
    assert upd(A + 4, B, 4) == -1 and "16-byte aligned" in lib.last_error()
    assert upd(A, B + 4, 4) == -1 and "16-byte aligned" in lib.last_error()
    assert upd(A, B, 4, st=S + 4) == -1 and "8-byte aligned" in lib.last_error()
    assert upd(A, A + 16, 8) == -1 and "overlap" in lib.last_error()
    assert upd(A, B, 4, d=1.5) == -1 and "[0, 1]" in lib.last_error()
    assert upd(A, B, 4, d=float("nan")) == -1 and "[0, 1]" in lib.last_error()
    swap = lambda p, e, n: so.adnm_ema_swap(p, e, n, None)
    assert swap(None, B, 4) == -1 and "null pointer" in lib.last_error()
    assert swap(A, None, 4) == -1 and "null pointer" in lib.last_error()
    assert swap(A, B, 0) == -1 and "multiple of 4" in lib.last_error()
    assert swap(A, B, 6) == -1 and "multiple of 4" in lib.last_error()
    assert swap(A + 4, B, 4) == -1 and "16-byte aligned" in lib.last_error()
    assert swap(A, A, 4) == -1 and "overlap" in lib.last_error()
    assert swap(A + 16, A, 8) == -1 and "overlap" in lib.last_error()


def test_ema_is_a_keyword_of_the_trainer_and_off_by_default():
    from adnm_hip.trainer import FlatTrainer
    sig = inspect.signature(FlatTrainer.__init__).parameters
    assert sig["ema_decay"].default is None and sig["ema_warmup"].default is True
    tr = FlatTrainer(None, None)
    assert tr.ema_decay is None and tr.ema is None and tr._ema_info is None
    assert "ema_decay" not in tr._scalars() and "ema_warmup" not in tr._scalars()
    with pytest.raises(RuntimeError, match="without ema_decay"):
        tr.ema_info()
    with pytest.raises(RuntimeError, match="without ema_decay"):
        with tr.ema_weights():
            pass
    for bad in (-0.1, 1.5, "0.9", True, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            FlatTrainer(None, None, ema_decay=bad)
    on = FlatTrainer(None, None, ema_decay=0.999, ema_warmup=False)
    assert on.ema_info() == {"decay": 0.0, "updates": 0}   # nothing has run: no device is touched
    assert on._scalars()["ema_decay"] == 0.999 and on._scalars()["ema_warmup"] is False
    with pytest.raises(RuntimeError, match="flat buffers do not exist"):
        with on.ema_weights():
            pass
