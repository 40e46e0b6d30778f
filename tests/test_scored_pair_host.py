"""The scored-pair contract at the C boundary without a GPU (csrc/scored_pair.h: pair_check): the five entry points that score a strided
forecast against a contiguous target refuse the same mistakes with the same return code and the same words, each under its own name.
Fake addresses throughout: anything that reached a launch would fault, and the stream is never touched.  The limits that belong to one
family (pools, scales, powers of two, value_scale, 65 536 pixels) are pinned by that family's own host tests."""
import ctypes

import pytest

from adnm_hip import lib

FRAMES, T, H, W = 40, 20, 64, 64
THR = (ctypes.c_float * 4)(20, 30, 35, 40)
BASE = dict(pred=16, ss=T * H * W, fs=H * W, tgt=32, table=64, thr=THR, small=True, ws=128, ws_bytes=1 << 40, frames=FRAMES, T=T)


def _pool(a):
    tab = lib.i64_table([4, 4, 16, 8]) if a["small"] else None
    return (a["pred"], a["ss"], a["fs"], a["tgt"], a["table"], a["thr"], 4, 90.0, tab, 2, a["ws"], a["ws_bytes"], a["frames"], a["T"], H, W, None)


def _fss(a):
    tab = lib.i64_table([1, 33]) if a["small"] else None
    return (a["pred"], a["ss"], a["fs"], a["tgt"], a["table"], a["thr"], 4, 90.0, tab, 2, a["ws"], a["ws_bytes"], a["frames"], a["T"], H, W, None)


def _spectrum(a):
    return (a["pred"], a["ss"], a["fs"], a["tgt"], a["table"], 90.0, a["ws"], a["ws_bytes"], a["frames"], a["T"], H, W, None)


def _joint(a):
    return (a["pred"], a["ss"], a["fs"], a["tgt"], a["table"], 90.0, a["ws"], a["ws_bytes"], a["frames"], a["T"], H * W, None)


def _objects(a):
    return (a["pred"], a["ss"], a["fs"], a["tgt"], a["table"], a["thr"], 4, 90.0, 1, a["ws"], a["ws_bytes"], a["frames"], a["T"], H, W, None)


# entry point -> (its arguments from the shared ones, what a short workspace returns, a shape whose workspace is not empty and its query)
ENTRIES = {
    "adnm_valid_pool_accum": (_pool, -3, lambda: lib.query("adnm_valid_pool_accum_ws_bytes", FRAMES, T, H, W, 4, lib.i64_table([4, 4, 16, 8]), 2)),
    "adnm_valid_fss_accum": (_fss, -3, lambda: lib.query("adnm_valid_fss_accum_ws_bytes", FRAMES, T, H, W, 4, lib.i64_table([1, 33]), 2)),
    "adnm_valid_spectrum_accum": (_spectrum, -1, lambda: lib.query("adnm_valid_spectrum_accum_ws_bytes", FRAMES, T, H, W)),
    "adnm_valid_joint_accum": (_joint, -1, lambda: lib.query("adnm_valid_joint_accum_ws_bytes", FRAMES, T, H * W, 90.0)),
    "adnm_valid_objects_accum": (_objects, -1, lambda: lib.query("adnm_valid_objects_accum_ws_bytes", FRAMES, T, H, W, 4)),
}

# the further pointers each entry point hands to the shared check as present: thresholds, its small table, spectrum's workspace
OTHER_POINTERS = {
    "adnm_valid_pool_accum": (dict(thr=None), dict(small=False)),
    "adnm_valid_fss_accum": (dict(thr=None), dict(small=False)),
    "adnm_valid_spectrum_accum": (dict(ws=None),),
    "adnm_valid_joint_accum": (),
    "adnm_valid_objects_accum": (dict(thr=None),),
}

# the shared refusals: every one is ADNM_EINVAL
REFUSALS = [
    (dict(pred=None), "null pointer"), (dict(tgt=None), "null pointer"), (dict(table=None), "null pointer"),
    (dict(pred=18), "4-byte aligned"), (dict(tgt=34), "4-byte aligned"),
    (dict(table=68), "8-byte aligned"),
    (dict(T=0), "must divide frames"), (dict(T=7), "must divide frames"),
    (dict(frames=65540), "frames <= 65535"),
    (dict(fs=H * W - 1), "pred_frame_stride"), (dict(fs=-H * W), "pred_frame_stride"),
    (dict(ss=-1), "pred_sample_stride"),
]


def _call(entry, **kw):
    rc = getattr(lib.load(), entry)(*ENTRIES[entry][0](dict(BASE, **kw)))
    return rc, lib.last_error()


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_shared_refusals_are_the_same_for_every_entry_point(entry):
    name = entry[len("adnm_"):] + ": "
    for kw, text in REFUSALS + [(kw, "null pointer") for kw in OTHER_POINTERS[entry]]:
        rc, err = _call(entry, **kw)
        assert rc == -1 and text in err and err.startswith(name), (entry, kw, rc, err)


def test_a_shape_refusal_prints_what_the_entry_point_was_given():
    for entry in ENTRIES:
        _, err = _call(entry, frames=65540)
        assert "(got frames 65540 T 20 " in err, (entry, err)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_short_workspace_is_refused_with_the_entry_points_own_code(entry):
    _, ws_rc, query = ENTRIES[entry]
    need = query()
    assert need >= 0, "the shared shape is inside every entry point's limits"
    name = entry[len("adnm_"):] + ": "
    if need:
        rc, err = _call(entry, ws_bytes=need - 1)
        assert rc == ws_rc and "workspace" in err and str(need) in err and err.startswith(name), (entry, rc, err)
    # one byte less than nothing: refused as well where nothing is needed
    rc, err = _call(entry, ws_bytes=-1)
    assert rc == ws_rc and "workspace" in err and err.startswith(name), (entry, rc, err)


def test_the_frame_stride_message_names_the_frame_as_its_entry_point_does():
    for entry in ENTRIES:
        _, err = _call(entry, fs=H * W - 1)
        assert ("must be 0 or >= hw" if entry == "adnm_valid_joint_accum" else "must be 0 or >= H*W") in err, (entry, err)
