"""Seeded cases for the FLAC writer on streams of any length (tests/test_flac_write_any_host.py,
tests/test_gpu_flac_write_any.py and tests/golden/make_flac_write_any_golden.py): int16 PCM whose last block is anything
from 1 to 4096 samples, the smallest shapes at which the partition rule, the lane bounds and the MD5 padding can go wrong.

  cases()       -> [(name, int16 array)]   one stream each: every length of LENGTHS with every kind of KINDS
  ragged()      -> [int16 array] x 300     streams of random lengths from 1 to 9000, for one call
  check_tally() -> {choice: count}         asserts, on the restatement, that the set makes every choice the rule has
  SUBSET, RATES                            the cases the fixture also records at other rates than 48 000 Hz

Conditions on this file, not measurements: no case is left out of any comparison, and every tally count is at least 1.
"""
import functools

import numpy as np

import flac_write_any_ref as A

BLOCK = 4096
SEED = 0xF1AD
# every length from 1 to 40; around 48, 64, 80, 256 and a block; two blocks and a bit, three and an odd bit; lengths whose
# remainder mod 32 is 27, 28, 29 or 31, below a block (27, 28, 29, 31, 59, 60, 61, 63) and above one (the last four)
LENGTHS = tuple(range(1, 41)) + (47, 59, 60, 61, 63, 79, 80, 81, 255, 256, 257, 4095, 4097, 4098, 4099, 4100, 4101, 8198, 8216, 12345,
                                 4123, 4124, 4125, 4127)
KINDS = ("noise", "tone", "ramp", "const", "step")
MD5_RESTS = (27, 28, 29, 31)
RATE = 48000
RATES = (4000, 44100, 65535)
SUBSET_LENGTHS = (1, 2, 3, 5, 17, 18, 20, 24, 31, 257, 4097, 12345)


def _rng(*tag):
    return np.random.default_rng([SEED] + [int(t) for t in tag])


def make(kind, n, tag=0):
    """n samples of one kind.  The levels go round with the length, so that short blocks are met loud (VERBATIM) and quiet
    (FIXED at order 0, where n <= 4 leaves no other order)."""
    r = _rng(KINDS.index(kind), n, tag)
    i = np.arange(n)
    if kind == "noise":
        amp = (5, 700, 32767)[(n + tag) % 3]
        x = r.integers(-amp, amp + 1, n)
    elif kind == "tone":                        # smooth, with small noise: the higher predictor orders
        x = (300, 9000, 30000)[(n + tag) % 3] * np.sin(i * (2 * np.pi / float(r.uniform(40, 160))) + float(r.uniform(0, 6))) + r.integers(-2, 3, n)
    elif kind == "ramp":
        x = int(r.integers(-7, 8)) * i + int(r.integers(-2000, 2000))
    elif kind == "const":
        x = np.full(n, int(r.integers(-32768, 32768)))
    else:                                       # "step": a constant whose last sample differs (one sample: the constant alone)
        x = np.full(n, (0, 3, -1234)[(n + tag) % 3])
        x[-1] += int(r.choice((-1, 1))) * (1, 40, 9000)[(n // 3 + tag) % 3]
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _tail(n, kind, seed):
    """n samples whose level changes inside the block (so that a high partition order pays), summed up `kind` times (so
    that the predictor of that order fits)"""
    r = np.random.default_rng([SEED, 7, n, kind, seed])
    amp = np.where(np.arange(n) < n // 2, 40, 1) if seed % 2 == 0 else np.where((np.arange(n) * 4 // n) % 2 == 0, 1, 60)
    x = r.integers(-1, 2, n) * amp
    for _ in range(kind):
        x = np.cumsum(x)
    return np.clip(x, -32768, 32767).astype(np.int16)


# (samples, {kind: seeds}): blocks of 8, 12 and 24 samples, P = 3, 2 and 3, on which the choice without the rule that a
# partition is longer than the warm-up would take a partition order the format forbids (check_tally says so)
BINDING = ((8, {2: (7, 15), 3: (27, 55), 4: (123, 223)}), (12, {2: (28, 66), 3: (1, 5), 4: (3, 5)}), (24, {2: (44, 72), 3: (14, 16), 4: (2, 3)}))


@functools.lru_cache(maxsize=None)
def cases():
    out = [("%s%d" % (kind, n), make(kind, n)) for n in LENGTHS for kind in KINDS]
    for n, seeds in BINDING:
        for kind, ss in seeds.items():
            out.append(("bind%d_%d_%d" % (n, kind, ss[0]), _tail(n, kind, ss[0])))
            # ... and as the last block behind a block of silence
            out.append(("bind%d_%d_%d" % (n, kind, ss[1]), np.concatenate((np.zeros(BLOCK, np.int16), _tail(n, kind, ss[1])))))
    for _, x in out:
        x.setflags(write=False)
    assert all(any(n % 32 == r and n < BLOCK for n in LENGTHS) and any(n % 32 == r and n > BLOCK for n in LENGTHS) for r in MD5_RESTS)
    return out


@functools.lru_cache(maxsize=None)
def subset():
    return [(name, x) for name, x in cases() if x.size in SUBSET_LENGTHS]


@functools.lru_cache(maxsize=None)
def ragged():
    r = _rng(99)
    out = [make(KINDS[int(k)], int(n), 1 + j) for j, (n, k) in enumerate(zip(r.integers(1, 9001, 300), r.integers(0, len(KINDS), 300)))]
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def check_tally():
    """Counts, over the last blocks of cases() and ragged(), of every choice the general rule has; asserts each is met."""
    t = dict.fromkeys(["fixed_P%d" % P for P in range(5)] + ["p_equals_P_below_4", "candidate_excluded", "exclusion_changes_choice",
                                                              "short_fixed_order0", "short_verbatim", "short_constant",
                                                              "odd_n_size8", "odd_n_size16"], 0)
    for x in [c[1] for c in cases()] + list(ragged()):
        last = np.asarray(x[(x.size - 1) // BLOCK * BLOCK:], np.int64)
        n = last.size
        c = A.choose(last)
        if n % 2 == 1 and n <= 256:
            t["odd_n_size8"] += 1                               # the block size spelled out in 8 bits
        if n % 2 == 1 and 256 < n < BLOCK:
            t["odd_n_size16"] += 1                              # ... in 16
        if n <= 4:
            t["short_constant"] += c["kind"] == A.CONSTANT
            t["short_verbatim"] += c["kind"] == A.VERBATIM
            if c["kind"] == A.FIXED:
                assert c["order"] == 0
                t["short_fixed_order0"] += 1
        if c["kind"] != A.FIXED:
            continue
        assert c["p"] <= c["P"] == A.finest(n) and (n >> c["p"]) > c["order"] and len(c["k"]) == 1 << c["p"]
        t["fixed_P%d" % c["P"]] += 1
        t["p_equals_P_below_4"] += c["p"] == c["P"] < 4 and c["P"] > 0
        if any((n >> q) <= c["order"] for q in range(c["P"] + 1)):
            t["candidate_excluded"] += 1
            free = A.choose(last, constrain=False)
            t["exclusion_changes_choice"] += free["kind"] != A.FIXED or free["p"] != c["p"]
    assert all(v >= 1 for v in t.values()), t
    return t
