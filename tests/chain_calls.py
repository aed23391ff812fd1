"""The converter-to-encoder entry points called through ctypes with every output buffer pre-filled, so that a test sees what
a refused call has and has not written: dcs_encode_streams_at(_level), dcs_resample_streams(_level), dcs_level_streams and
dcs_encode_files(_level).  Each call returns a Call with the status, the dcs_last_error text read right after it and the
buffers as the library left them.  tests/test_gpu_chain_order.py asserts on them; tools/chain_hashes.py hashes them."""
import ctypes
from collections import namedtuple

import numpy as np

import dcsexplorer_amd as D
from dcsexplorer_amd import api as A
from dcsexplorer_amd.api import _ptr

FILL = 0xA5
Call = namedtuple("Call", "status msg out offs info linfo")


def filled(n, dtype):
    """n records of dtype, every byte FILL"""
    a = np.zeros(max(int(n), 1), dtype)
    a.view(np.uint8)[:] = FILL
    return a


def untouched(a, first=0):
    """True where no byte of a[first:] was written"""
    return bool((np.ascontiguousarray(a[first:]).view(np.uint8) == FILL).all())


def _streams(pcm_list, rates, channels):
    pcm, offs = A._encode_input(pcm_list)
    n = len(offs) - 1
    return pcm, offs, n, A._per_stream(rates, n, np.uint32, "rates"), A._per_stream(channels, n, np.int32, "channel counts")


def _level_args(level, n):
    """level: None, a Level, a list of Levels, or (pointer or None, nLevels) passed as it is"""
    if level is None:
        return None, 0
    if isinstance(level, tuple):
        return level
    return A._levels(level, n)


def _msg(ctx):
    return ctx.L.dcs_last_error(ctx.h).decode()


def enc_at(ctx, pcm_list, rates, version=0x9400, fmt=None, channels=1, at_unity=False, level=None, params=None, **kw):
    """dcs_encode_streams_at, or dcs_encode_streams_at_level where level is given; params: an EncodeParams to pass as it is"""
    p = params if params is not None else D.transcode_params(version, fmt, **kw)
    pcm, offs, n, r, ch = _streams(pcm_list, rates, channels)
    bound = D.encode_bound if version == 0x9400 else D.encode93_bound
    cap = sum(bound(A._resample_bound(int(offs[i + 1] - offs[i]), int(r[i]), int(ch[i]), at_unity)) or bound(65535 * 240) for i in range(n))
    out, out_offs, info, linfo = filled(cap, np.uint8), filled(n + 1, np.uint64), filled(n, A.ENCODE_INFO_DTYPE), filled(n, A.LEVEL_INFO_DTYPE)
    args = (ctx.h, _ptr(pcm), _ptr(offs), n, _ptr(r), _ptr(ch), None, A.RESAMPLE_AT_UNITY if at_unity else 0, ctypes.byref(p), _ptr(out),
            cap, _ptr(out_offs), _ptr(info))
    if level is None:
        st = ctx.L.dcs_encode_streams_at(*args)
    else:
        lv, n_lv = _level_args(level, n)
        st = ctx.L.dcs_encode_streams_at_level(*args, lv, n_lv, _ptr(linfo))
    return Call(st, _msg(ctx), out, out_offs, info[:n], linfo[:n])


def resample(ctx, pcm_list, rates, channels=1, at_unity=False, level=None, short=0):
    """dcs_resample_streams_level (levels NULL, 0 where level is None); short: floats the capacity lacks"""
    pcm, offs, n, r, ch = _streams(pcm_list, rates, channels)
    need = sum(D.resample_count(int(offs[i + 1] - offs[i]), int(r[i]), int(ch[i]), at_unity=at_unity) for i in range(n))
    out, out_offs, linfo = filled(need, np.float32), filled(n + 1, np.uint64), filled(n, A.LEVEL_INFO_DTYPE)
    lv, n_lv = _level_args(level, n)
    st = ctx.L.dcs_resample_streams_level(ctx.h, _ptr(pcm), _ptr(offs), n, _ptr(r), _ptr(ch), None, A.RESAMPLE_AT_UNITY if at_unity else 0,
                                          _ptr(out), need - short, _ptr(out_offs), lv, n_lv, _ptr(linfo))
    return Call(st, _msg(ctx), out, out_offs, None, linfo[:n])


def level_streams(ctx, pcm_list, level, short=0):
    """dcs_level_streams; short: floats the capacity lacks"""
    pcm, offs = A._encode_input(pcm_list)
    n = len(offs) - 1
    out, out_offs, linfo = filled(int(offs[-1]), np.float32), filled(n + 1, np.uint64), filled(n, A.LEVEL_INFO_DTYPE)
    lv, n_lv = _level_args(level, n)
    st = ctx.L.dcs_level_streams(ctx.h, _ptr(pcm), _ptr(offs), n, lv, n_lv, _ptr(out), int(offs[-1]) - short, _ptr(out_offs), _ptr(linfo))
    return Call(st, _msg(ctx), out, out_offs, None, linfo[:n])


def encode_files(ctx, files, version=0x9400, fmt=None, at_unity=False, level=None, short=0, **kw):
    """dcs_encode_files, or dcs_encode_files_level where level is given; short: bytes the capacity lacks of what the call
    needs (taken from a first call with the plan's bound)"""
    p = D.transcode_params(version, fmt, **kw)
    blob, offs = A._files_blob(files)
    n = len(offs) - 1
    flags = A.RESAMPLE_AT_UNITY if at_unity else 0
    bound = np.zeros(max(n, 1), np.uint64)
    st = ctx.L.dcs_encode_files_plan(_ptr(blob), _ptr(offs), n, ctypes.byref(p), None, flags, None, _ptr(bound), None)
    cap = int(bound[:n].sum()) if st == 0 else 0

    def call(cap):
        out, out_offs = filled(cap, np.uint8), filled(n + 1, np.uint64)
        info, linfo = filled(n, A.ENCODE_FILE_INFO_DTYPE), filled(n, A.LEVEL_INFO_DTYPE)
        args = (ctx.h, _ptr(blob), _ptr(offs), n, ctypes.byref(p), None, flags, _ptr(out), cap, _ptr(out_offs), _ptr(info))
        if level is None:
            st = ctx.L.dcs_encode_files(*args)
        else:
            lv, n_lv = _level_args(level, n)
            st = ctx.L.dcs_encode_files_level(*args, lv, n_lv, _ptr(linfo))
        return Call(st, _msg(ctx), out, out_offs, info[:n], linfo[:n])

    c = call(cap)
    if short and c.status == 0:
        c = call(int(c.offs[n]) - short)
    return c
