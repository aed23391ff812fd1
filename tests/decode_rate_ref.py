"""A numpy restatement of the library's output-rate converter (dcs_resample_out_streams, and what dcs_decode_streams_at does
to the decoder's PCM): libsamplerate's sinc converter, mono, at the ratio out_rate / 31250.0, run with the reference
encoder's call pattern (16 samples per src_process call, a 512-float output buffer, one zero-length end-of-input call with
its 512-sample cap), between libsamplerate's own two conversions (samplerate.c:486-516):

    in   src_short_to_float_array   (float)(s / 32768.0), exact for every int16
    out  src_float_to_short_array   v = (double)y * 2^31; v >= 2147483647.0 -> 32767; v <= -2147483648.0 -> -32768; else
                                    (short)(lrint(v) >> 16): an arithmetic shift, so it floors.  libsamplerate's choice.

What of resample_ref.py does not fix the ratio is used from there (buffer_len, the half sums); the parameters, the walk
and the conversions are restated here.  The walk rounds with Python's round(), which rounds halves to even as rint does,
and remembers its results: a decode list has few distinct lengths."""
import functools

import numpy as np

import resample_ref as R

FLUSH_CAP = R.FLUSH_CAP
AT_UNITY = R.AT_UNITY
MIN_RATE, MAX_RATE = 4000, 65535
IN_RATE = 31250.0


def pass_through(out_rate, flags):
    return out_rate == 31250 and not (flags & AT_UNITY)


def params(n_coeffs, increment, out_rate):
    """(half_filter_chan_len, 1 / ratio, terminate, float_increment, increment_t) at ratio out_rate / 31250.0
    (src_sinc.c:359-405)"""
    ratio = float(out_rate) / IN_RATE
    count = (n_coeffs - 2 + 2.0) / increment
    if ratio < 1.0:
        count /= ratio
    half = round(count) + 1
    float_inc = increment * (ratio if ratio < 1.0 else 1.0)
    return half, 1.0 / ratio, 1.0 / ratio + 1e-20, float_inc, round(float_inc * 4096.0)


def walk(n, n_coeffs, increment, out_rate):
    pos, sfi = _walk(int(n), int(n_coeffs), int(increment), int(out_rate), FLUSH_CAP)
    return pos.copy(), sfi.copy()


@functools.lru_cache(maxsize=256)
def _walk(n, n_coeffs, increment, out_rate, flush_cap):
    """the integer input position and start_filter_index of every output of a stream of n samples: sinc_mono_vari_process's
    position chain over the encoder's calls, the converter's buffer in its own indices (see resample_ref.walk)"""
    half, step, terminate, float_inc, _ = params(n_coeffs, increment, out_rate)
    b_len = R.buffer_len(n_coeffs, increment)
    b_cur = b_end = 0
    b_real_end = -1
    pos, idx, fed = 0, 0.0, 0
    out_pos, out_sfi = [], []

    def advance():
        nonlocal b_cur, pos, idx
        rem = idx - float(round(idx))       # fmod_one (common.h:147-155)
        if rem < 0.0:
            rem += 1.0
        adv = round(idx - rem)
        b_cur = (b_cur + adv) % b_len
        pos += adv
        idx = rem

    while b_real_end < 0:
        in_count = min(16, n - fed)
        eof = in_count == 0
        fed += in_count
        in_used = out_gen = 0
        advance()                           # the call's opening fmod_one
        while out_gen < flush_cap:
            if (b_end - b_cur + b_len) % b_len <= half:
                if b_real_end < 0:          # prepare_data
                    if b_cur == 0:
                        ln = b_len - 2 * half
                        b_cur = b_end = half
                    elif b_end + half + 1 < b_len:
                        ln = max(b_len - b_cur - half, 0)
                    else:
                        ln = b_end - b_cur
                        b_cur, b_end = half, half + ln
                        ln = max(b_len - b_cur - half, 0)
                    ln = min(in_count - in_used, ln)
                    b_end += ln
                    in_used += ln
                    if in_used == in_count and b_end - b_cur < 2 * half and eof:
                        if b_len - b_end < half + 5:
                            ln = b_end - b_cur
                            b_cur, b_end = half, half + ln
                        b_real_end = b_end
                        ln = half + 5
                        if b_end + ln > b_len:
                            ln = b_len - b_end
                        b_end += ln
                if (b_end - b_cur + b_len) % b_len <= half:
                    break
            if b_real_end >= 0 and float(b_cur) + idx + terminate > float(b_real_end):
                break
            out_pos.append(pos)
            out_sfi.append(round(idx * float_inc * 4096.0))
            out_gen += 1
            idx += step
            advance()
    return np.array(out_pos, np.int64), np.array(out_sfi, np.int64)


def count(n, out_rate, n_coeffs, increment, flags=0):
    return n if pass_through(out_rate, flags) else len(walk(n, n_coeffs, increment, out_rate)[0])


def short_to_float(pcm):
    """src_short_to_float_array"""
    return (np.asarray(pcm, np.int16).astype(np.float64) / 32768.0).astype(np.float32)


def float_to_short(y):
    """src_float_to_short_array -> (int16 samples, how many the two clamping branches took)"""
    v = np.asarray(y, np.float32).astype(np.float64) * 2147483648.0
    hi, lo = v >= 2147483647.0, v <= -2147483648.0
    mid = ~(hi | lo)
    out = np.empty(len(v), np.int16)
    out[hi] = 32767
    out[lo] = -32768
    out[mid] = (np.rint(v[mid]).astype(np.int64) >> 16).astype(np.int16)
    return out, int(hi.sum() + lo.sum())


def convert_float(pcm, out_rate, coeffs, increment):
    """the converter's float output for int16 input (never a pass-through)"""
    x = short_to_float(pcm)
    c = np.asarray(coeffs, dtype=np.float32)
    n_coeffs = len(c)
    pos, sfi = walk(len(x), n_coeffs, increment, out_rate)
    if len(pos) == 0:
        return np.zeros(0, np.float32)
    _, _, _, float_inc, inc_t = params(n_coeffs, increment, out_rate)
    max_fi = (n_coeffs - 2) << 12
    reach = max_fi // inc_t + 2
    xp = np.concatenate([np.zeros(reach, np.float32), x, np.zeros(reach + 2, np.float32)])
    p = pos + reach
    left = R._half_sum(c, xp, p, sfi, inc_t, max_fi, +1)
    right = R._half_sum(c, xp, p, inc_t - sfi, inc_t, max_fi, -1)
    with np.errstate(over="ignore"):
        return ((float_inc / increment) * (left + right)).astype(np.float32)


def convert_float_many(pcms, out_rate, coeffs, increment):
    """convert_float of several streams at once -> a list of float32 arrays.  The streams lie one behind the other, each
    between zeros of its own as wide as the filter reaches, and each half sum runs once over the taps for the outputs of all
    of them: per output the products, their order and the sums are convert_float's (tests with many short streams and a
    long filter spend their time per tap, not per output)."""
    c = np.asarray(coeffs, dtype=np.float32)
    n_coeffs = len(c)
    _, _, _, float_inc, inc_t = params(n_coeffs, increment, out_rate)
    max_fi = (n_coeffs - 2) << 12
    reach = max_fi // inc_t + 2
    parts, ps, sfis, counts, at = [], [], [], [], 0
    for pcm in pcms:
        x = short_to_float(pcm)
        pos, sfi = walk(len(x), n_coeffs, increment, out_rate)
        parts += [np.zeros(reach, np.float32), x, np.zeros(reach + 2, np.float32)]
        ps.append(pos + at + reach)
        sfis.append(sfi)
        counts.append(len(pos))
        at += len(x) + 2 * reach + 2
    if sum(counts) == 0:
        return [np.zeros(0, np.float32) for _ in pcms]
    xp, p, sfi = np.concatenate(parts), np.concatenate(ps), np.concatenate(sfis)
    left = R._half_sum(c, xp, p, sfi, inc_t, max_fi, +1)
    right = R._half_sum(c, xp, p, inc_t - sfi, inc_t, max_fi, -1)
    with np.errstate(over="ignore"):
        y = ((float_inc / increment) * (left + right)).astype(np.float32)
    return np.split(y, np.cumsum(counts)[:-1])


def convert(pcm, out_rate, coeffs, increment, flags=0):
    """dcs_resample_out_streams for one stream -> (int16 samples, info) with info = dict(nIn, nOut, nClipped, peak), peak
    the float32 largest |y| of the converter's output (a pass-through: of s / 32768)"""
    pcm = np.asarray(pcm, np.int16)
    if pass_through(out_rate, flags):
        y = short_to_float(pcm)
        out, clipped = pcm.copy(), 0
    else:
        y = convert_float(pcm, out_rate, coeffs, increment)
        out, clipped = float_to_short(y)
    peak = np.float32(np.max(np.abs(y))) if len(y) else np.float32(0.0)
    return out, dict(nIn=len(pcm), nOut=len(out), nClipped=clipped, peak=peak)


# ------------------------------------------------------------------------------------------------ the tests' signals
def lcg16(seed, n):
    """n int16 values every machine computes to the same bits: a 32-bit LCG's top 16 bits"""
    v = seed & 0xFFFFFFFF
    out = np.empty(n, np.int64)
    for i in range(n):
        v = (1664525 * v + 1013904223) & 0xFFFFFFFF
        out[i] = v >> 16
    return (out - 32768).astype(np.int16)


def signal(kind, n, seed=1):
    """silence, dc+ / dc- (DC at +-32767), impulse, square (+-32767, period 100 samples: the clip case), noise"""
    if kind == "silence":
        return np.zeros(n, np.int16)
    if kind == "dc+":
        return np.full(n, 32767, np.int16)
    if kind == "dc-":
        return np.full(n, -32767, np.int16)
    if kind == "impulse":
        x = np.zeros(n, np.int16)
        x[n // 2] = 32767
        return x
    if kind == "square":
        return np.where((np.arange(n) // 50) & 1, -32767, 32767).astype(np.int16)
    if kind == "noise":
        return lcg16(seed, n)
    raise ValueError(kind)


def case_pcm(key):
    """a fixture case's input from its recipe "<kind>:<n>:<seed>" """
    kind, n, seed = key.split(":")
    return signal(kind, int(n), int(seed))
