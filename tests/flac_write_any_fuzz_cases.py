"""Seeded int16 streams for the fuzz of the any-length FLAC writer (dcs_flac_write_samples) against the compiled libFLAC
(tests/test_flac_write_any_vs_reference.py, tests/test_gpu_flac_write_any_vs_reference.py): streams whose last block is
not a multiple of 16 samples, the branch of fwChooseKernel and fwWriteKernel with P = ctz(n) < 4 (half-wavefront sums joined
in LDS, lane loops bounded by n, fwChooseFrom<false>), with the content families of tests/flac_write_fuzz_cases.py, which
asserts whole frames on every stream and so never reaches that branch.  Recipes only; no samples are committed.

  sets() -> {family: [(stream name, int16 array)]}     one dcs_flac_write_samples call a family

Last blocks: for each P in 0 .. 3 lengths from both ends of the range (LAST: below 64 samples, where a partition has fewer
samples than its group has lanes, and near 4096), and a few of whole 16s as controls; each alone and behind one and two
full blocks (the placements rotate over a family's streams, and every length meets all three).  Content, placed by the
LAST block's start and length: +-1 / +-2 / +-3 noise with and without DC (ties between orders and parameters); noise of
every amplitude 2^0 .. 2^15 (a Rice parameter each); a constant that changes at positions 0 .. 4 and n-5 .. n-1; ramps and
parabolas with +-1 noise; a level step at every partition boundary j (n >> p), p <= P; +-1 noise summed two, three and four
times and rounded sines (the higher orders); full-scale alternation in both phases and with one hole, full-scale noise and
signs (the kernel bounds a half-wavefront's sum at 32 lanes x 16 residuals below 2^21 on this shape); one spike at each of
the block's first and last 5 samples; the blocks of tests/flac_write_any_cases.py on which the rule that a partition is
longer than the warm-up binds; the oracle's PCM of seeded synthetic DCS streams of all six layouts, cut at a seeded odd
length.

check_tally() states, on the restatement (flac_write_any_ref.choose) over the last blocks with n & 15 != 0, that the input
makes every choice the branch has.  Conditions on the input, checked on the CPU."""
import collections
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import flac_write_any_cases as AC       # noqa: E402
import flac_write_any_ref as A          # noqa: E402

BLOCK = A.BLOCK
SEED = 0xF1AD7
RATE = 44100
# last-block lengths by P = ctz(n); CONTROLS are whole 16s (the other branch)
LAST = {0: (4095, 4093, 33, 5), 1: (4094, 34, 6), 2: (4092, 36, 12), 3: (4088, 40, 24, 8)}
CONTROLS = (4096, 4080, 48, 16)
LENGTHS = tuple(n for P in sorted(LAST) for n in LAST[P]) + CONTROLS
assert all(A.finest(n) == P for P, ns in LAST.items() for n in ns) and all(n % 16 == 0 for n in CONTROLS)


def _rng(*tag):
    return np.random.default_rng([SEED] + [int(t) for t in tag])


def _i16(x):
    return np.clip(np.asarray(x, np.int64), -32768, 32767).astype(np.int16)


def _noise(r, n, a):
    return r.integers(-a, a + 1, n)


# A family: (r, total, base, n) -> [(variant name, int64 samples of the whole stream)], base and n the last block's start
# and length.  The blocks in front carry the family's content too.

def _low_noise(r, total, base, n):
    return [("noise%d_dc%d" % (a, dc), _noise(r, total, a) + dc) for a in (1, 2, 3) for dc in (0, 12345)]


def _amplitudes(r, total, base, n):
    return [("noise_2^%d" % e, _noise(r, total, 1 << e)) for e in range(16)]


def _edge_positions(n):
    return sorted({p for p in list(range(5)) + list(range(n - 5, n)) if 0 <= p < n})


def _constant_change(r, total, base, n):
    out = []
    for pos in _edge_positions(n):
        x = np.full(total, int(r.integers(-30000, 30000)), np.int64)
        x[base + pos:] += int(r.choice([-1, 1, 2, -300, 20000]))
        out.append(("const_change_at%d" % pos, x))
    return out


def _ramps(r, total, base, n):
    out = []
    i = np.arange(total, dtype=np.int64) % BLOCK
    for rep in range(4):
        a, b, c = int(r.integers(-3, 4)), int(r.integers(-2000, 2000)), [0, 0, 1, -1][rep]
        out.append(("ramp%d" % rep, b + a * i + c * (i * i >> int(r.integers(9, 13))) + _noise(r, total, 1) * (rep != 0)))
    return out


def _partition_steps(r, total, base, n):
    """+-1 noise whose amplitude steps at boundary j (n >> p) of the last block, for every p <= P and every j (the boundaries
    of p < P are among those of P); a block that cannot be split (P = 0) steps at its middle"""
    P = A.finest(n)
    out = []
    for j in range(1, 1 << P) if P else (0,):
        at = j * (n >> P) if P else n // 2
        amp = np.ones(total, np.int64)
        loud = int(r.choice([40, 60, 900]))
        if j % 2:
            amp[base + at:] = loud
        else:
            amp[:base + at] = loud
        x = _noise(r, total, 1) * amp
        for _ in range(int(r.integers(0, 3))):
            x = np.cumsum(x)
        out.append(("step_at%d_of_P%d" % (at, P), x))
    return out


def _summed(r, total, base, n):
    out = []
    for kind, run in ((2, 240), (3, 60), (4, 30)):
        x = _noise(r, total + run, 1)[:(total + run) // run * run].reshape(-1, run)
        for _ in range(kind):
            x = np.cumsum(x, axis=1)
        out.append(("summed%d" % kind, x.ravel()[:total]))
    for rep, (amp, lo, hi) in enumerate(((300.0, 12, 400), (30000.0, 30, 120), (3000.0, 12, 400))):
        w = 2 * np.pi / float(r.uniform(lo, hi))
        out.append(("sine%d" % rep, np.rint(amp * np.sin(np.arange(total) * w + float(r.uniform(0, 6))))))
    return out


def _full_scale(r, total, base, n):
    i = np.arange(total)
    hole = np.where(i & 1, -32768, 32767)
    hole[base + int(r.integers(n))] = 0
    return [("alternate", np.where(i & 1, -32768, 32767)), ("alternate_neg", np.where(i & 1, 32767, -32768)), ("alternate_one_hole", hole),
            ("fullscale_noise", r.integers(-32768, 32768, total)), ("fullscale_signs", np.where(r.random(total) < 0.5, -32768, 32767))]


def _spikes(r, total, base, n):
    out = []
    for pos in _edge_positions(n):
        x = np.zeros(total, np.int64)
        x[base + pos] = int(r.choice([1, -1, 2, 32767, -32768, 100]))
        out.append(("spike_at%d" % pos, x))
    return out


FAMILIES = (("low_noise", _low_noise), ("amplitudes", _amplitudes), ("constant_change", _constant_change), ("ramps", _ramps),
            ("partition_steps", _partition_steps), ("summed", _summed), ("full_scale", _full_scale), ("spikes", _spikes))


def _binding():
    """flac_write_any_cases' blocks of 8, 12 and 24 samples on which the choice without the partition-longer-than-warm-up rule
    would take a partition order the format forbids: alone, and behind one and two blocks of quiet noise"""
    out = []
    r = _rng(20)
    for n, seeds in AC.BINDING:
        for kind, ss in seeds.items():
            for fronts, s in enumerate(ss + ss[:1]):
                out.append(("bind%d_%d_%d_behind%d" % (n, kind, s, fronts), np.concatenate((_i16(_noise(r, fronts * BLOCK, 2)), AC._tail(n, kind, s)))))
    return out


def _synth():
    import dcsexplorer_amd as D
    from oracle.dcs_oracle import Oracle
    oracle, r, out = Oracle(), _rng(21), []
    for fmt in range(6):
        for rep in range(2):
            frames = int(r.integers(3, 40))
            s = D.synth_stream(fmt, frames, seed=int(r.integers(1 << 30)), nbands=18 if fmt == D.FMT_93A_T1 else 16)
            pcm = np.ascontiguousarray(oracle.decode(D.format_os(fmt), 255, [s], [0x64], frames + 2), np.int16).ravel()
            cut = int(r.integers(pcm.size // 2, pcm.size)) | 1
            out.append(("synth%d_%d_cut%d" % (fmt, rep, cut), pcm[:cut].copy()))
    return out


@functools.lru_cache(maxsize=None)
def sets():
    out = collections.OrderedDict()
    for f, (family, fn) in enumerate(FAMILIES):
        items = []
        for k, n in enumerate(LENGTHS):
            # the variants of one (family, length) are drawn for each placement from that placement's own generator
            made = {fronts: fn(_rng(f, n, fronts), fronts * BLOCK + n, fronts * BLOCK, n) for fronts in range(3)}
            for v in range(len(made[0])):
                fronts = (v + k + f) % 3
                name, x = made[fronts][v]
                items.append(("%s/%s_n%d_behind%d" % (family, name, n, fronts), _i16(x)))
        out[family] = items
    out["binding"] = _binding()
    out["synth"] = _synth()
    for items in out.values():
        for _, x in items:
            assert x.dtype == np.int16 and x.size >= 1
            x.setflags(write=False)
    names = [n for items in out.values() for n, _ in items]
    assert len(set(names)) == len(names)
    return out


def streams():
    return [s for items in sets().values() for s in items]


def last_block(x):
    return np.asarray(x[(x.size - 1) // BLOCK * BLOCK:], np.int64)


def fillers():
    """one-sample and 240-sample streams put between the streams of the shuffled call"""
    r = _rng(30)
    return [np.array([-7], np.int16), _i16(r.integers(-200, 200, 240)), np.array([32767], np.int16), _i16(np.arange(240) * 9)]


def shuffled(n):
    """-> (order, how many fillers go in front of each)"""
    r = _rng(31)
    return [int(x) for x in r.permutation(n)], [int(x) for x in r.integers(0, 3, n)]


@functools.lru_cache(maxsize=None)
def check_tally():
    """Counts, over the last blocks with n & 15 != 0, of every choice the branch has; asserts each is at least 1 and that every
    length of LAST comes alone and behind one and two full blocks."""
    t = collections.Counter()
    placed = collections.Counter()
    for name, x in streams():
        last = last_block(x)
        n = last.size
        placed[n, (x.size - 1) // BLOCK] += 1
        if n & 15 == 0:
            t["control"] += 1
            continue
        c = A.choose(last)
        t[("CONSTANT", "VERBATIM", "FIXED")[[A.CONSTANT, A.VERBATIM, A.FIXED].index(c["kind"])]] += 1
        if c["kind"] != A.FIXED:
            continue
        assert c["p"] <= c["P"] == A.finest(n) < 4 and (n >> c["p"]) > c["order"] and len(c["k"]) == 1 << c["p"]
        t["order%d" % c["order"]] += 1
        t["P%d_p%d" % (c["P"], c["p"])] += 1
        for k in c["k"]:
            t["k%d" % k] += 1
        if any((n >> q) <= c["order"] for q in range(c["P"] + 1)):
            t["candidate_excluded"] += 1
            free = A.choose(last, constrain=False)
            t["exclusion_changes_choice"] += free["kind"] != A.FIXED or free["p"] != c["p"]
    need = (["control", "CONSTANT", "VERBATIM", "FIXED", "candidate_excluded", "exclusion_changes_choice"] + ["order%d" % o for o in range(5)]
            + ["P%d_p%d" % (P, p) for P in range(4) for p in range(P + 1)] + ["k%d" % k for k in range(15)])
    assert len([k for k in need if k.startswith("P")]) == 10
    missing = [k for k in need if t[k] < 1]
    assert not missing, (missing, dict(t))
    assert all(placed[n, fronts] >= 1 for n in LENGTHS for fronts in range(3)), placed
    return {k: t[k] for k in need}
