"""Seeded cases for the FLAC writer (tests/test_flac_write_host.py, tests/test_gpu_flac_write.py and
tests/golden/make_flac_write_golden.py): int16 PCM in whole DCS frames of 240 samples, the smallest shapes at which block,
offset and header logic can go wrong.

  cases()   -> [(name, int16 array)]                   one stream each
  shapes()  -> [(name, pool of int16 arrays, index)]   many streams in one call; stream i is pool[index[i]]
  streams() -> [(name, (os, bytes, volume, level))]    the six layouts' synthetic DCS streams
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FRAME = 240
BLOCK = 4096
SEED = 0xF1AC


def _rng(tag):
    return np.random.default_rng([SEED, tag])


def _sine(n, amp, period, noise, tag):
    r = _rng(tag)
    x = amp * np.sin(np.arange(n) * (2 * np.pi / period)) + r.integers(-noise, noise + 1, n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _bursts(n, every, length, tag):
    """digital silence with a short burst of a sine every `every` samples"""
    x = np.zeros(n, np.int16)
    r = _rng(tag)
    for start in range(every // 3, n - length, every):
        x[start:start + length] = _sine(length, int(r.integers(100, 20000)), float(r.uniform(20, 200)), 2, tag + start)
    return x


def _tail(n, kind, seed):
    """n samples whose level changes inside the block (so that a high partition order pays), summed up `kind` times (so
    that the predictor of that order fits)"""
    r = np.random.default_rng([SEED, 7, n, kind, seed])
    amp = np.where(np.arange(n) < n // 2, 40, 1) if seed % 2 == 0 else np.where((np.arange(n) // (n // 4)) % 2 == 0, 1, 60)
    x = r.integers(-1, 2, n) * amp
    for _ in range(kind):
        x = np.cumsum(x)
    return np.clip(x, -32768, 32767).astype(np.int16)


# (frames, samples of the last block, seeds per kind 1..4): streams of 239, 222 and 205 frames end in a block of 16, 32 and
# 48 samples, where a partition of the higher partition orders is no longer than the predictor's warm-up.  The seeds hold,
# for every length, tails on which the choice without that rule would take a partition order the format forbids
# (tests/test_flac_write_host.py says which).
SHORT_TAILS = ((239, 16, {1: (0, 1), 2: (0, 1), 3: (0, 1), 4: (1, 3, 6)}), (222, 32, {1: (0, 1), 2: (0, 187), 3: (10, 65, 158), 4: (19, 36)}),
               (205, 48, {1: (0, 1), 2: (0, 1), 3: (3, 4), 4: (2, 4, 5)}))


def streams():
    import dcsexplorer_amd as D
    out = []
    for fmt in range(6):
        s = D.synth_stream(fmt, 33, seed=SEED + fmt, nbands=18 if fmt == D.FMT_93A_T1 else 16)
        out.append(("synth%d" % fmt, (D.format_os(fmt), s, 255, 0x64)))
    return out


@functools.lru_cache(maxsize=None)
def _synth_pcm():
    """the six layouts' streams decoded by the oracle with two extra frames: 35 frames each"""
    from oracle.dcs_oracle import Oracle
    oracle = Oracle()
    return [(name, np.ascontiguousarray(oracle.decode(os_, vol, [s], [lvl], 35), np.int16).ravel())
            for name, (os_, s, vol, lvl) in streams()]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # lengths in frames: one short block with the 8-bit and the 16-bit size code, a block and a bit, two and a bit,
    # frame numbers in two and in three bytes
    for frames in (1, 17, 18, 35):
        out.append(("len%d" % frames, _sine(frames * FRAME, 9000, 61.7, 6, frames)))
    out.append(("len2200", _bursts(2200 * FRAME, 37 * BLOCK + 100, 700, 2200)))
    out.append(("len35000", _bursts(35000 * FRAME, 293 * BLOCK + 1000, 900, 35000)))
    n = 35 * FRAME
    i = np.arange(n)
    r = _rng(1)
    out.append(("silence", np.zeros(n, np.int16)))
    out.append(("const_min", np.full(n, -32768, np.int16)))
    out.append(("alternating", np.where(i & 1, -32768, 32767).astype(np.int16)))
    out.append(("white", r.integers(-32768, 32768, n).astype(np.int16)))
    out.append(("noise3", r.integers(-3, 4, n).astype(np.int16)))
    out.append(("ramp", (3 * i - 12000).astype(np.int16)))
    for amp in (30, 1000, 30000):
        out.append(("sine%d" % amp, _sine(n, amp, 97.3, 1, amp)))
    spike = np.zeros(n, np.int16)
    spike[BLOCK + 1234] = 32767
    out.append(("spike", spike))
    # segments of the above, switching away from the block boundaries
    seg = np.concatenate([np.zeros(1000, np.int16), out[9][1][:3000], np.full(777, 1234, np.int16), out[10][1][:2500],
                          (3 * np.arange(500) - 700).astype(np.int16), _sine(623, 20000, 31.0, 40, 77)])
    assert seg.size == n
    out.append(("segments", seg))
    # one block each, cut from a burst of len35000: their frames hold a run of zeros that ends in the last bit of a 64-bit
    # window at one of the four byte alignments a frame can lie at (a reader that shifts its window by 64 there goes wrong)
    for shift in (2, 4, 8):
        at = 684 * BLOCK + shift
        out.append(("zeros63_%d" % shift, out[5][1][at:at + 17 * FRAME].copy()))
    # silence that ends in a short last block (SHORT_TAILS), and the 16 samples of four values that make order 1 with the
    # finest partitions the cheapest
    for frames, n, seeds in SHORT_TAILS:
        for kind, ss in seeds.items():
            for seed in ss:
                x = np.zeros(frames * FRAME, np.int16)
                x[-n:] = _tail(n, kind, seed)
                out.append(("tail%d_%d_%d" % (n, kind, seed), x))
    x = np.zeros(239 * FRAME, np.int16)
    x[-16:] = [20000, 28000, 28000, 20000] * 4
    out.append(("tail16_square", x))
    out.extend(_synth_pcm())
    for name, x in out:
        assert x.dtype == np.int16 and x.size % FRAME == 0 and x.size >= FRAME, name
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def shapes():
    r = _rng(2)
    # 300 streams of 1..40 frames: offsets and ragged streams
    ragged = [_sine(int(f) * FRAME, int(a), float(p), 3, 1000 + k)
              for k, (f, a, p) in enumerate(zip(r.integers(1, 41, 300), r.integers(0, 12000, 300), r.uniform(8, 300, 300)))]
    # 70 000 streams of one frame, more than 65 535 blocks in a launch: a pool of sixteen frames, dealt at random
    pool = [_sine(FRAME, 400 * k, 23.0 + k, k % 5, 2000 + k) for k in range(16)]
    return [("ragged300", ragged, np.arange(300)), ("one_frame_70000", pool, r.integers(0, 16, 70000))]
