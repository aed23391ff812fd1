"""Seeded int16 streams for the fuzz of the FLAC writer (tests/test_flac_write_vs_reference.py,
tests/test_gpu_flac_write_vs_reference.py): whole frames of 240 samples, with content chosen for the ties and thresholds of
the writer's discrete choices (the best of five fixed orders, a Rice parameter per partition, the partition order, CONSTANT /
VERBATIM / FIXED), where a GPU reduction and the numpy restatement (tests/flac_write_ref.py) could part ways.

  sets() -> {name: [(stream name, int16 array)]}     one dcs_flac_write_streams call a set

Lengths: 1 to 60 frames; the lengths whose last block is 16, 32, ... 240 samples (15 L = m mod 256: 239, 222, 205, 188 ... 1
frames) and 4080 samples (17 and 273 frames); the set `lengths` holds every one of them, the others draw from them.
Content: noise of +-1, +-2, +-3 with and without a DC offset; constants that change value once inside a block, at each of
positions 0 to 4 and n-5 to n-1; ramps and parabolas with +-1 noise; level steps at the partition boundaries of every partition
order; full-scale alternation and full-scale noise; one spike at each of a block's first and last 5 samples; silence with one
nonzero sample; +-1 noise summed up two to four times and rounded sines (the higher fixed orders); noise of every amplitude 2^0 .. 2^15 (a Rice parameter each); the oracle's PCM of seeded synthetic DCS streams
of all six layouts.

(The order-4 residual of a 4096-sample block sums to at most 4092 x 8 x 65535 = 2 145 353 760, which full-scale alternation
reaches: 0.099 % below 2^31, the nearest an int16 block comes to it.)"""
import collections
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import flac_write_ref as R          # noqa: E402

FRAME, BLOCK = 240, 4096
SEED = 0xF1AC6
SHORT_LAST = [(239 * m) % 256 for m in range(1, 16)]                    # last block of 16 m samples
LENGTHS = list(range(1, 61)) + [f for f in SHORT_LAST if f > 60] + [273]  # (17 frames: a last and only block of 4080)
assert all((f * FRAME) % BLOCK == 16 * m for m, f in enumerate(SHORT_LAST, 1)) and (17 * FRAME) % BLOCK == (273 * FRAME) % BLOCK == 4080


def _rng(*tag):
    return np.random.default_rng([SEED, *tag])


def _i16(x):
    return np.clip(np.asarray(x, np.int64), -32768, 32767).astype(np.int16)


def _last_block(n):
    """(start, size) of a stream's last block"""
    size = n % BLOCK or BLOCK
    return n - size, size


@functools.lru_cache(maxsize=None)
def sets():
    out = collections.OrderedDict()

    def add(name, items):
        for _, x in items:
            assert x.dtype == np.int16 and x.size % FRAME == 0 and x.size >= FRAME
            x.setflags(write=False)
        out[name] = items

    # every length, low noise: ties between orders and parameters at every last-block size
    items = []
    for k, f in enumerate(LENGTHS):
        r = _rng(1, f)
        a = 1 + k % 3
        items.append(("len%d_noise%d" % (f, a), _i16(r.integers(-a, a + 1, f * FRAME) + (0 if k % 2 else 1000))))
    add("lengths", items)

    r = _rng(2)
    pick = lambda: int(r.choice(LENGTHS[:64]))
    items = []
    for a in (1, 2, 3):
        for dc in (0, -7, 12345):
            for rep in range(3):
                f = pick()
                items.append(("noise%d_dc%d_%d" % (a, dc, rep), _i16(r.integers(-a, a + 1, f * FRAME) + dc)))
    for e in range(16):                                                  # a Rice parameter each
        f = pick()
        items.append(("noise_2^%d" % e, _i16(r.integers(-(1 << e), (1 << e) + 1, f * FRAME))))
    add("noise", items)

    # a constant that changes value once inside a block (the CONSTANT decision), first block and last block
    items = []
    for f in (1, 17, 18, 35, 239, 222):
        n = f * FRAME
        start, size = _last_block(n)
        for base, bsize in dict.fromkeys(((0, min(n, BLOCK)), (start, size))):
            for pos in list(range(5)) + list(range(bsize - 5, bsize)):
                x = np.full(n, int(r.integers(-30000, 30000)), np.int64)
                x[base + pos:] += int(r.choice([-1, 1, 2, -300, 20000]))
                items.append(("const_change_%d_at%d+%d" % (f, base, pos), _i16(x)))
    add("constant_change", items)

    # ramps and parabolas with +-1 noise: adjacent fixed orders tie
    items = []
    for rep in range(40):
        f = pick()
        i = np.arange(f * FRAME, dtype=np.int64) % BLOCK
        a, b, c = int(r.integers(-3, 4)), int(r.integers(-2000, 2000)), [0, 0, 1, -1][rep % 4]
        x = b + a * i + c * (i * i >> int(r.integers(9, 13))) + r.integers(-1, 2, i.size) * (rep % 3 != 0)
        items.append(("ramp%d" % rep, _i16(x)))
    add("ramps", items)

    # level steps at the partition boundaries of every partition order, in a full and in a short last block
    items = []
    for f in (18, 35, 222, 205, 188, 1, 8):
        n = f * FRAME
        for base, bsize in dict.fromkeys(((0, min(n, BLOCK)), _last_block(n))):
            for p in range(1, 5):
                if bsize % (1 << p):
                    continue
                for at in sorted(set(int(v) for v in r.integers(1, 1 << p, 2))):
                    amp = np.ones(n, np.int64)
                    lo_, hi_ = base + at * (bsize >> p), base + min(1 << p, at + 1 + int(r.integers(2))) * (bsize >> p)
                    amp[lo_:hi_] = int(r.choice([40, 60, 900]))
                    x = r.integers(-1, 2, n) * amp
                    for _ in range(int(r.integers(0, 3))):
                        x = np.cumsum(x)
                    items.append(("step_%d_at%d_p%d_%d" % (f, base, p, at), _i16(x)))
    for rep in range(30):                                               # a level step in the middle of every block: partition order 1
        f = pick()
        n = f * FRAME
        amp = np.ones(n, np.int64)
        for b in range(0, n, BLOCK):
            size = min(BLOCK, n - b)
            half = slice(b, b + size // 2) if rep % 2 else slice(b + size // 2, b + size)
            amp[half] = int(r.choice([30, 200, 3000]))
        items.append(("halves_%d" % rep, _i16(r.integers(-1, 2, n) * amp)))
    add("partition_steps", items)

    # +-1 noise summed up two, three and four times in short runs: the higher fixed orders, by narrow margins
    items = []
    for kind, run in ((2, 240), (3, 60), (4, 30)):
        for rep in range(16):
            f = pick()
            x = r.integers(-1, 2, (f * FRAME // run, run))
            for _ in range(kind):
                x = np.cumsum(x, axis=1)
            items.append(("summed%d_%d" % (kind, rep), _i16(x.ravel())))
    # rounded sines: order k's residual is about A w^k against rounding noise that grows with k, so amplitude and period set
    # which of orders 2, 3 and 4 wins, and by how little
    for rep in range(70):
        f = pick()
        amp, w = float(r.choice([300, 3000, 30000])), 2 * np.pi / float(r.uniform(12, 400))
        if rep >= 40:                                                   # (order 4's corner)
            amp, w = 30000.0, 2 * np.pi / float(r.uniform(30, 120))
        x = np.rint(amp * np.sin(np.arange(f * FRAME) * w + float(r.uniform(0, 6))))
        items.append(("sine%d" % rep, _i16(x)))
    add("summed", items)

    # full scale: the order-4 residual sums of a block reach their maximum
    items = []
    for f in (18, 35, 52, 17):
        n = f * FRAME
        i = np.arange(n)
        items.append(("alternate_%d" % f, np.where(i & 1, -32768, 32767).astype(np.int16)))
        items.append(("alternate_neg_%d" % f, np.where(i & 1, 32767, -32768).astype(np.int16)))
        items.append(("fullscale_noise_%d" % f, r.integers(-32768, 32768, n).astype(np.int16)))
        items.append(("fullscale_signs_%d" % f, np.where(r.random(n) < 0.5, -32768, 32767).astype(np.int16)))
        x = np.where(i & 1, -32768, 32767)
        x[int(r.integers(n))] = 0
        items.append(("alternate_one_hole_%d" % f, x.astype(np.int16)))
    add("full_scale", items)

    # one spike at each of a block's first and last 5 samples; silence with one nonzero sample
    items = []
    for f in (18, 239, 17):
        n = f * FRAME
        for base, bsize in dict.fromkeys(((0, min(n, BLOCK)), _last_block(n))):
            for pos in list(range(5)) + list(range(bsize - 5, bsize)):
                x = np.zeros(n, np.int16)
                x[base + pos] = int(r.choice([1, -1, 2, 32767, -32768, 100]))
                items.append(("spike_%d_at%d+%d" % (f, base, pos), x))
    for rep in range(12):
        f = pick()
        x = np.zeros(f * FRAME, np.int16)
        x[int(r.integers(x.size))] = int(r.choice([1, -1, 3, -32768]))
        items.append(("silence_one_%d" % rep, x))
    add("spikes", items)

    # decoded PCM of seeded synthetic DCS streams, all six layouts
    import dcsexplorer_amd as D
    from oracle.dcs_oracle import Oracle
    oracle = Oracle()
    items = []
    for fmt in range(6):
        for rep in range(3):
            frames = int(r.integers(3, 40))
            s = D.synth_stream(fmt, frames, seed=int(r.integers(1 << 30)), nbands=18 if fmt == D.FMT_93A_T1 else 16)
            pcm = np.ascontiguousarray(oracle.decode(D.format_os(fmt), 255, [s], [0x64], frames + 2), np.int16).ravel()
            items.append(("synth%d_%d" % (fmt, rep), pcm))
    add("synth", items)
    names = [n for items in out.values() for n, _ in items]
    assert len(set(names)) == len(names)
    return out


def fillers():
    """one-frame streams put between the streams of a shuffled call"""
    r = _rng(9)
    return [_i16(r.integers(-200, 200, FRAME)), np.zeros(FRAME, np.int16), _i16(np.arange(FRAME) * 9)]


def shuffled(n, tag):
    """-> (order, how many one-frame fillers go in front of each)"""
    r = _rng(10, tag)
    return [int(x) for x in r.permutation(n)], [int(x) for x in r.integers(0, 3, n)]


def tally(streams):
    """what the restatement chose, per block of every stream: kinds, fixed orders, partition orders, Rice parameters"""
    kinds, orders, pos, ks = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    for _, x in streams:
        s = np.asarray(x, np.int64)
        for b in range(0, s.size, BLOCK):
            c = R.choose(s[b:b + BLOCK])
            kinds[("CONSTANT", "VERBATIM", "FIXED")[[R.CONSTANT, R.VERBATIM, R.FIXED].index(c["kind"])]] += 1
            if c["kind"] == R.FIXED:
                orders[c["order"]] += 1
                pos[c["p"]] += 1
                ks.update(c["k"])
    return kinds, orders, pos, ks


def check_tally(streams):
    """print the counts and require every choice: each kind, fixed order and partition order 20 times, each Rice parameter once"""
    kinds, orders, pos, ks = tally(streams)
    print("\nblocks by kind:", dict(kinds), "\nfixed orders:", dict(sorted(orders.items())), "\npartition orders:", dict(sorted(pos.items())),
          "\nRice parameters:", dict(sorted(ks.items())))
    assert all(kinds[k] >= 20 for k in ("CONSTANT", "VERBATIM", "FIXED")), kinds
    assert all(orders[o] >= 20 for o in range(5)), orders
    assert all(pos[p] >= 20 for p in range(5)), pos
    assert all(ks[k] >= 1 for k in range(15)), ks
