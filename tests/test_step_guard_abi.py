"""The entry points of the monitored step at the C boundary, without a GPU: declared in include/adnm_hip.h, exported by the library,
additive (they left the ABI version as it was), and validating their arguments before any launch."""
import ctypes
import inspect

import pytest

from adnm_hip import lib

NEW = ("adnm_step_guard", "adnm_adamw_step_guarded", "adnm_quant_update_guarded", "adnm_loss_stat")


def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
        assert protos[name][0] == "int" and protos[name][1][-1] == "adnm_stream_t"
    assert lib.load().adnm_abi_version() == 11
    # the guarded optimiser is adnm_adamw_step without its workspace (no second norm pass), plus the statistics block
    plain, guarded = protos["adnm_adamw_step"][1], protos["adnm_adamw_step_guarded"][1]
    assert len(guarded) == len(plain) - 2 + 1 and guarded[-2] == "const void*"


def test_arguments_are_checked_on_the_host():
    so = lib.load()
    assert so.adnm_step_guard(None, 4, None, 0.0, None, None, 0, None, None) == -1 and "null pointer" in lib.last_error()
    assert so.adnm_step_guard(16, 6, 16, 0.0, None, 16, 1 << 20, 16, None) == -1 and "multiple of 4" in lib.last_error()
    assert so.adnm_step_guard(16, 4, 16, 0.0, None, 16, 1 << 20, 12, None) == -1 and "8-byte aligned" in lib.last_error()
    assert so.adnm_step_guard(16, 4, 16, 0.0, None, 16, 8, 16, None) == -3 and "workspace" in lib.last_error()
    assert so.adnm_adamw_step_guarded(16, 16, 16, 16, 4, 16, 1e-3, 0.9, 0.999, 1e-9, 1e-2, 0.0, None, 0, None, None, 0, None, None, None, None) == -1
    assert "null pointer" in lib.last_error()
    assert so.adnm_adamw_step_guarded(16, 16, 16, 16, 4, 16, 1e-3, 0.9, 0.999, 1e-9, 1e-2, 0.0, 16, 3, None, None, 0, None, None, 16, None) == -1
    assert "shadow" in lib.last_error()
    assert so.adnm_quant_update_guarded(16, 1, 16, 2.0, None, None) == -1 and "bad arguments" in lib.last_error()
    assert so.adnm_quant_update_guarded(16, 1, 16, 0.5, 16, None) == -1 and "headroom" in lib.last_error()
    assert so.adnm_loss_stat(None, 16, None) == -1 and "null pointer" in lib.last_error()
    assert so.adnm_loss_stat(18, 16, None) == -1 and "misaligned" in lib.last_error()


def test_monitor_is_a_keyword_of_the_trainer_and_off_by_default():
    from adnm_hip.trainer import FlatTrainer
    assert inspect.signature(FlatTrainer.__init__).parameters["monitor"].default is False
    tr = FlatTrainer(None, None)
    assert tr.monitor is False and tr._stats is None
    with pytest.raises(RuntimeError, match="monitor=False"):
        tr.stats()
    with pytest.raises(RuntimeError, match="monitor=False"):
        tr.reset_stats()
    idle = FlatTrainer(None, None, monitor=True).stats()   # nothing has run: nothing counted, and no device is touched
    assert idle["steps"] == 0 and idle["skipped"] == 0 and idle["norm_mean"] == 0.0 and idle["clip_rate"] == 0.0
    assert set(idle) == {"steps", "skipped", "loss_sum", "loss_nonfinite", "norm_sum", "norm_mean", "norm_max", "last_norm", "clip_count", "clip_rate"}
