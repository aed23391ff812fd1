"""A numpy restatement of the library's resampler (dcs_resample_streams), written from the reference: EncodeFile's stereo
downmix (DCSEncodeFile.cpp:81-102), then libsamplerate's sinc converter, mono, at the fixed ratio 31250.0 / rate
(DCSEncoder.cpp:165-185; src_sinc.c:280-424 sinc_mono_vari_process and calc_output_single; common.h:147-155 fmod_one),
with the 512-sample cap of CloseStream's end-of-input call (DCSEncoder.cpp:717-721).

The position chain is walked serially in Python floats (IEEE doubles, as the C code); each output's two half sums are
vectorised across outputs, one tap at a time, so every sum keeps the C order.  numpy does not contract a * b + c."""
import numpy as np

FLUSH_CAP = 512
AT_UNITY = 1
MIN_RATE, MAX_RATE = 4000, 384000


def lcg_signal(seed, n, amp):
    """a long test signal that every machine computes to the same bits: a 32-bit LCG's top 24 bits, centred and scaled (the
    long fixture cases keep only this recipe, not their samples)"""
    x = np.empty(n, np.uint32)
    v = np.uint64(seed & 0xFFFFFFFF)
    # x[i] = (1664525 * x[i-1] + 1013904223) mod 2^32, in blocks: a[k] x + c[k] advances k steps at once
    block = 4096
    a = np.empty(block, np.uint64)
    c = np.empty(block, np.uint64)
    a[0], c[0] = 1664525, 1013904223
    for k in range(1, block):
        a[k] = (a[k - 1] * np.uint64(1664525)) & np.uint64(0xFFFFFFFF)
        c[k] = (c[k - 1] * np.uint64(1664525) + np.uint64(1013904223)) & np.uint64(0xFFFFFFFF)
    for i in range(0, n, block):
        m = min(block, n - i)
        x[i:i + m] = ((a[:m] * v + c[:m]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        v = np.uint64(x[i + m - 1])
    u = (x >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / (1 << 24)) - np.float32(0.5)
    return u * np.float32(amp)


def fixture_pcm(arrays, key):
    """a fixture case's input: arrays[key + "/pcm"], or the recipe lcg:<seed>:<n>:<amp>"""
    if key.startswith("lcg:"):
        _, seed, n, amp = key.split(":")
        return lcg_signal(int(seed), int(n), float(amp))
    return arrays[key + "/pcm"]


def downmix(values, channels):
    """EncodeFile's loop: (L + R) / 2.0f per pair, a final unpaired value alone"""
    x = np.asarray(values, dtype=np.float32)
    if channels == 1:
        return x.copy()
    m = len(x) // 2
    out = np.empty((len(x) + 1) // 2, np.float32)
    out[:m] = (x[0:2 * m:2] + x[1:2 * m:2]) / np.float32(2.0)
    if len(x) & 1:
        out[m] = x[-1]
    return out


def pass_through(rate, flags):
    return rate == 31250 and not (flags & AT_UNITY)


def params(n_coeffs, increment, rate):
    """(half_filter_chan_len, 1 / ratio, terminate, float_increment, increment_t) for one stream (src_sinc.c:359-405)"""
    ratio = 31250.0 / rate
    count = (n_coeffs - 2 + 2.0) / increment
    if ratio < 1.0:
        count /= ratio
    half = int(np.rint(count)) + 1
    float_inc = increment * (ratio if ratio < 1.0 else 1.0)
    return half, 1.0 / ratio, 1.0 / ratio + 1e-20, float_inc, int(np.rint(float_inc * 4096.0))


def fmod_one(x):
    res = x - float(np.rint(x))
    return res + 1.0 if res < 0.0 else res


def buffer_len(n_coeffs, increment):
    """the converter's buffer length (sinc_set_converter: 2.5 * coeff_half_len / increment * SRC_MAX_RATIO, at least 4096)"""
    return max(int(np.rint(2.5 * (n_coeffs - 2) / (increment * 1.0) * 256)), 4096)


def walk(n, n_coeffs, increment, rate):
    """the integer input position and start_filter_index of every output of a stream of n mono samples.

    The calls are the reference encoder's: 16 samples per src_process call, a 512-float output buffer, then one zero-length
    end-of-input call.  The buffer is restated in its own indices (prepare_data's loads and moves, the ring's length) because
    the end rule compares b_current + input_index + terminate with b_real_end in those indices, and that f64 sum rounds by the
    size of b_current.  Everything else depends only on the absolute position."""
    half, step, terminate, float_inc, _ = params(n_coeffs, increment, rate)
    b_len = buffer_len(n_coeffs, increment)
    b_cur = b_end = 0
    b_real_end = -1
    pos, idx, fed = 0, 0.0, 0
    out_pos, out_sfi = [], []
    while b_real_end < 0:
        in_count = min(16, n - fed)
        eof = in_count == 0
        fed += in_count
        in_used = out_gen = 0
        rem = fmod_one(idx)                 # the start of sinc_mono_vari_process (no move: idx is in [0, 1) already)
        adv = int(np.rint(idx - rem))
        b_cur = (b_cur + adv) % b_len
        pos += adv
        idx = rem
        while out_gen < FLUSH_CAP:
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
            out_sfi.append(int(np.rint(idx * float_inc * 4096.0)))
            out_gen += 1
            idx += step
            rem = fmod_one(idx)
            adv = int(np.rint(idx - rem))
            b_cur = (b_cur + adv) % b_len
            pos += adv
            idx = rem
    return np.array(out_pos, np.int64), np.array(out_sfi, np.int64)


def count(n_values, rate, n_coeffs, increment, channels=1, flags=0):
    n = (n_values + 1) // 2 if channels == 2 else n_values
    return n if pass_through(rate, flags) else len(walk(n, n_coeffs, increment, rate)[0])


def _half_sum(c, xp, pos, start_fi, increment, max_fi, sign):
    """one half of calc_output_single for every output at once: sign +1 = the left half (data index rising, loop while
    filter_index >= 0), -1 = the right half (falling, while > 0)"""
    cc = (max_fi - start_fi) // increment
    fi = start_fi + cc * increment
    d = pos - cc if sign > 0 else pos + 1 + cc
    acc = np.zeros(len(pos), np.float64)
    live = np.ones(len(pos), bool)
    while live.any():
        indx = np.where(live, fi >> 12, 0)
        fraction = (fi & 4095).astype(np.float64) * (1.0 / 4096.0)
        c0, c1 = c[indx], c[indx + 1]
        icoeff = c0.astype(np.float64) + fraction * (c1 - c0).astype(np.float64)
        acc = np.where(live, acc + icoeff * xp[np.where(live, d, 0)].astype(np.float64), acc)
        fi = fi - increment
        d = d + sign
        live &= (fi >= 0) if sign > 0 else (fi > 0)
    return acc


def convert(mono, rate, coeffs, increment, flags=0):
    """the converter on mono float32 samples -> float32 at 31 250 Hz"""
    x = np.asarray(mono, dtype=np.float32)
    if pass_through(rate, flags):
        return x.copy()
    c = np.asarray(coeffs, dtype=np.float32)
    n_coeffs = len(c)
    pos, sfi = walk(len(x), n_coeffs, increment, rate)
    if len(pos) == 0:
        return np.zeros(0, np.float32)
    _, _, _, float_inc, inc_t = params(n_coeffs, increment, rate)
    max_fi = (n_coeffs - 2) << 12
    # x with its zeros: indices from -reach .. n + reach
    reach = max_fi // inc_t + 2
    xp = np.concatenate([np.zeros(reach, np.float32), x, np.zeros(reach + 2, np.float32)])
    p = pos + reach
    left = _half_sum(c, xp, p, sfi, inc_t, max_fi, +1)
    right = _half_sum(c, xp, p, inc_t - sfi, inc_t, max_fi, -1)
    with np.errstate(over="ignore"):        # a sum past FLT_MAX rounds to +-inf, as the C cast does
        return ((float_inc / increment) * (left + right)).astype(np.float32)


def resample(values, rate, coeffs, increment, channels=1, flags=0):
    """dcs_resample_streams for one stream"""
    return convert(downmix(values, channels), rate, coeffs, increment, flags)
