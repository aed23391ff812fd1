"""Seeded FLAC files for the fuzz of the reader against the compiled libFLAC (tests/test_flac_vs_reference.py,
tests/test_gpu_flac_vs_reference.py, tools/flac_walk_sanitize.sh), and the compiled checker itself (test infrastructure).
Every case is a recipe: a seed that produces bytes through flac_cases.make_frame; no FLAC bytes are committed.

  well_formed() -> [Case]     files the format allows, drawn per frame and per channel: depth 8 / 16 / 24, mono and stereo, the
                              assignments 0 1 8 9 10, wasted bits (side channels too), block sizes 1 2 15 16 17 31 32 33 192, odd
                              sizes in both blockings, every size code, a short last block; const, verbatim, fixed 0-4 and LPC of
                              order 1-32 (the block size and the first partition's length among them), precision 1-15, shift 0-15;
                              samples at the depth's limits (the 25-bit side channel too); both Rice methods, every partition
                              order the block allows, a parameter per partition, escapes of width 0 up to 31, an empty first
                              partition; unary runs of 33-64, 65-128 and more than 128 bits, begun at each of 32 consecutive bit
                              positions; every rate code; frame numbers in 1-3 bytes and sample numbers in 1-4; metadata blocks,
                              an ID3v2 prefix, the trailers the rules accept
  damaged()     -> [Damaged]  seeded mutations of the small well-formed files, the CRC-8 and CRC-16 made right again (a share
                              keeps the broken CRC): bit flips in the first subframe's header, its LPC parameters, its partition
                              header and in residual bits, a frame shorter or longer by a byte, a wrong frame number, a STREAMINFO
                              total off by a block
  compositions(n, seed)       the orders and fillers a GPU test runs a set in: a frame's alignment in the uploaded bytes is set
                              by everything before it in the call

The signal comes first here (the encoder's direction): a channel's samples are drawn, the predictor's residuals follow from
them, and flac_cases.S(exact=...) writes exactly those, so no recipe can leave its depth and nothing caps a residual.
(Frame numbers in 4 bytes would take 65 536 frames in one file; they are left to the sample numbers.)

check_load() / check_md5() run oracle/_ref/dcs_flacref and dcs_flacref_san (`make -C oracle flacref`)."""
import collections
import functools
import hashlib
import os
import re
import struct
import subprocess
import tempfile

import numpy as np

import flac_cases as F
import flac_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
EXE, EXE_SAN = os.path.join(REF_DIR, "dcs_flacref"), os.path.join(REF_DIR, "dcs_flacref_san")
MISSING = "oracle/_ref/dcs_flacref* not built (needs /root/reference; `make -C oracle flacref`)"
SEED = 0xF1AC5
N_RANDOM = 264              # 44 files for each of the six (depth, channels) classes
N_DAMAGED = 240
KEEP_VALUES = 1 << 16       # loads up to this many values keep their bits; all keep the sha256
RUN_CLASSES = ("33-64", "65-128", ">128")
TYPES = ("const", "verbatim", "fixed0", "fixed1", "fixed2", "fixed3", "fixed4", "lpc")

Case = collections.namedtuple("Case", "name data ints fmt types runs parts")
Damaged = collections.namedtuple("Damaged", "name data source mutation crc_fixed")
Load = collections.namedtuple("Load", "kind channels rate count sha256 values text reports value_shifts")
# libFLAC 1.3.1 sign-extends and scales with `<<` on signed values all over its decoder (bitreader.c read_raw_int32, fixed.c,
# the wasted bits and the side channel in stream_decoder.c), so -fsanitize=shift speaks on nearly every file there is.  ISO C
# leaves a left shift of a negative value, or one into the sign bit, undefined; GCC, which builds the checker, defines it
# ("GCC does not use the latitude given in C99 and C11 only to treat certain aspects of signed << as undefined", Integers
# implementation), and both builds give the same floats.  Those reports are counted (value_shifts) and do not set a file
# aside.  Every other report does: a shift by the type's width or more (read_raw_int32 of an escape of width 0 shifts by 32,
# which the hardware and the optimiser are free to answer differently), an index out of bounds, a float out of an int's range.
VALUE_SHIFT = re.compile(r"left shift of (negative value -?\d+|\d+ by \d+ places cannot be represented in type)")


# ------------------------------------------------------------------------------------------------------------- channels

def _signed_width(r):
    return 0 if r == 0 else (r.bit_length() if r > 0 else (-r - 1).bit_length()) + 1


def _run_class(span):
    return None if span < 33 else RUN_CLASSES[0] if span <= 64 else RUN_CLASSES[1] if span <= 128 else RUN_CLASSES[2]


def _signal(rng, bs, eff, mode, shrink):
    lo, hi = -(1 << (eff - 1)), (1 << (eff - 1)) - 1
    if mode == "edge":                                      # within a few counts of the limits, in stretches
        top = rng.random(bs) < 0.5
        if rng.random() < 0.5:
            top = np.repeat(rng.random((bs + 3) // 4) < 0.5, 4)[:bs]
        d = rng.integers(0, 4, bs)
        return [int(hi - x) if t else int(lo + x) for t, x in zip(top, d)]
    if mode == "quiet":
        a, b = ((0, 0), (-1, 0), (-1, 1), (-2, 2))[int(rng.integers(4))]
        return [int(x) for x in rng.integers(a, b + 1, bs)]
    e = max(1, int(rng.integers(1, eff)) - 2 * shrink)
    amp = (1 << e) - 1
    if mode == "walk":
        x = np.cumsum(rng.integers(-max(1, amp >> 4), max(1, amp >> 4) + 1, bs))
        return [int(v) for v in np.clip(x, -amp - 1, amp)]
    return [int(x) for x in rng.integers(-amp - 1, amp + 1, bs)]


def _lpc(rng, bs, eff):
    top = min(32, bs)
    pick = rng.random()
    fits = [bs >> p for p in range(16) if (bs >> p) << p == bs and 1 <= bs >> p <= top]
    order = int(rng.choice(fits)) if pick < 0.3 and fits else top if pick < 0.4 else int(rng.integers(1, top + 1))
    prec = int(rng.choice([1, 2, 15, int(rng.integers(1, 16))]))
    shift = int(rng.choice([0, 15, int(rng.integers(0, 16))]))
    c = rng.integers(-(1 << (prec - 1)), 1 << (prec - 1), order).astype(np.int64)
    total, limit = int(np.abs(c).sum()), 1 << (28 - eff + shift)          # |residual| stays below 2^29
    if total > limit:
        c = np.sign(c) * (np.abs(c) * limit // total)
    return order, prec, shift, [int(x) for x in c]


def _runs_residuals(rng, bs, order, eff, k):
    """fixed order 0 or 1 and a small Rice parameter: small residuals, and a few whose unary run is long"""
    lo, hi = -(1 << (eff - 1)), (1 << (eff - 1)) - 1
    res, data = [], [0] * order
    want = set(int(x) for x in rng.integers(0, max(1, bs - order), int(rng.integers(1, 5))))
    for i in range(bs - order):
        prev = data[-1] if order else 0
        if i in want:
            span = int(rng.choice([int(rng.integers(33, 65)), 64, int(rng.integers(65, 129)), 128, int(rng.integers(129, 400))]))
            u = ((span - 1) << k) | int(rng.integers(0, 1 << k))
            u = min(u, 2 * hi - 2)
        else:
            u = int(rng.integers(0, 3))
        cands = [(u >> 1) ^ -(u & 1), ((u ^ 1) >> 1) ^ -((u ^ 1) & 1), 0]
        r = next((c for c in cands if lo <= prev + c <= hi), -prev)
        res.append(r)
        data.append(prev + r)
    return data[:order], res


def _partitions(rng, res, counts, method):
    kmax = 30 if method else 14
    ks, i = [], 0
    for c in counts:
        part = res[i:i + c]
        i += c
        umax = max([(r << 1) if r >= 0 else ((-r) << 1) - 1 for r in part] or [0])
        need, pick = umax.bit_length(), rng.random()
        width = max([_signed_width(r) for r in part] or [0])
        if pick < 0.2 or need - kmax > 8:
            ks.append(("esc", min(31, width + int(rng.choice([0, 0, 1, 2])))))
        elif pick < 0.3:
            ks.append(kmax)
        elif pick < 0.4 and need <= 8:
            ks.append(0)
        else:
            ks.append(max(0, min(kmax, need - 1 - int(rng.choice([0, 1, 2, 3, 6])))))
    return ks


def _channel(rng, bs, depth, shrink, target=None, cheap=False):
    """-> (recipe, the channel's samples as coded, before the assignment is undone, type tag, run classes)"""
    w = 0
    if target is None and rng.random() < 0.3:
        w = int(rng.integers(1, min(depth - 2, 7) + 1))
    eff = depth - w
    lo, hi = -(1 << (eff - 1)), (1 << (eff - 1)) - 1
    t = ("const", "verbatim", "fixed", "lpc")[int(rng.choice(4, p=[0.08, 0.12, 0.4, 0.4]))]
    mode = ("walk", "noise", "edge", "quiet", "runs")[int(rng.choice(5, p=[0.2, 0.2, 0.2, 0.1, 0.3]))]
    if cheap:
        t, mode = ("const", "verbatim", "fixed")[int(rng.integers(3))], "walk"
    if target is not None and t == "const" and len(set(target)) > 1:
        t = "verbatim"
    if t == "const":
        v = target[0] if target is not None else int(rng.choice([hi - int(rng.integers(3)), lo + int(rng.integers(3)), int(rng.integers(lo, hi + 1))]))
        v = max(lo, min(hi, v >> (2 * shrink)))
        return F.S("const", wasted=w, values=[v << w]), [v << w] * bs, "const", set()
    sig = list(target) if target is not None else _signal(rng, bs, eff, "walk" if mode == "runs" and t == "verbatim" else mode, shrink)
    if t == "verbatim":
        return F.S("verbatim", wasted=w, values=[x << w for x in sig]), [x << w for x in sig], "verbatim", set()
    method = int(rng.integers(2))
    if t == "fixed" or mode == "runs" or cheap:
        t = "fixed"
        order = min(bs, int(rng.integers(2)) if mode == "runs" or cheap else int(rng.integers(5)))
        prec, shift, coefs = 0, 0, F.FIXED_TAPS[order]
    else:
        order, prec, shift, coefs = _lpc(rng, bs, eff)
    pos = [p for p in range(16) if (bs >> p) << p == bs and bs >> p >= max(order, 1)]
    if cheap:
        pos = pos[:4]
    po = pos[-1] if rng.random() < 0.4 else int(rng.choice(pos))
    counts = F._partition_counts(bs, order, po)
    if mode == "runs" and target is None:
        k = int(rng.integers(0, 3))
        while k and (400 << k) > hi:
            k -= 1
        warm, res = _runs_residuals(rng, bs, order, eff, k)
        ks = [k] * len(counts)
    else:
        warm, res = sig[:order], []
        for i in range(order, bs):
            res.append(sig[i] - (sum(coefs[j] * sig[i - 1 - j] for j in range(order)) >> shift))
        ks = _partitions(rng, res, counts, method)
    data = list(warm)
    for r in res:
        data.append(r + (sum(coefs[j] * data[-1 - j] for j in range(order)) >> shift))
    runs, i = set(), 0
    for c, k in zip(counts, ks):
        if not isinstance(k, tuple):
            for r in res[i:i + c]:
                cls = _run_class(((((r << 1) if r >= 0 else ((-r) << 1) - 1)) >> k) + 1)
                if cls:
                    runs.add(cls)
        i += c
    spec = F.S(t, order=order, prec=prec, shift=shift, method=method, po=po, k=ks, wasted=w, exact=(warm, coefs, res))
    return spec, [x << w for x in data], "lpc" if t == "lpc" else "fixed%d" % order, runs


def _fields(hdr_len, spec, depth, bs):
    """the bit ranges of channel 0's fields inside the frame: {name: (first bit, width)}"""
    w = spec["wasted"]
    eff = depth - w
    at = 8 * hdr_len
    out = {"subframe_header": (at, 8 + w)}
    at += 8 + w
    if spec["t"] in ("fixed", "lpc"):
        at += eff * spec["order"]
        if spec["t"] == "lpc":
            out["lpc_parameters"] = (at, 9 + spec["prec"] * spec["order"])
            out["lpc_shift"] = (at + 4, 1)                   # the shift's sign
            at += 9 + spec["prec"] * spec["order"]
        out["partition_header"] = (at, 6 + (5 if spec["method"] else 4))
        at += 6 + (5 if spec["method"] else 4)
    out["residual"] = (at, None)
    return out


def _frame(rng, number, bs, bits, channels, variable, cheap=False):
    """-> ((bytes, channels), channel 0's fields, type tags, run classes)"""
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    assign = 0 if channels == 1 else int(rng.choice([1, 8, 9, 10]))
    for shrink in range(12):
        if shrink >= 10:
            assign = 1 if channels == 2 else 0
        side = [(assign == 8 and c == 1) or (assign == 9 and c == 0) or (assign == 10 and c == 1) for c in range(channels)]
        targets = [None] * channels
        if assign >= 8 and not cheap and rng.random() < 0.35:          # the side channel at its own limits: L and R at opposite ones
            L, Rr = _signal(rng, bs, bits, "edge", 0), _signal(rng, bs, bits, "edge", 0)
            s = [a - b for a, b in zip(L, Rr)]
            targets = {8: [L, s], 9: [s, Rr], 10: [[(a + b) >> 1 for a, b in zip(L, Rr)], s]}[assign]
        made = [_channel(rng, bs, bits + (1 if side[c] else 0), shrink, targets[c], cheap) for c in range(channels)]
        chans = [m[1] for m in made]
        if channels == 2:
            chans = list(F.undo_assignment(assign, chans[0], chans[1]))
        if all(lo <= x <= hi for c in chans for x in c):
            break
    else:
        raise AssertionError("no frame whose channels fit their depth")
    code = F.block_size_code(bs)
    hdr = dict(variable=variable, rate_code=int(rng.choice([0, int(rng.integers(1, 15))])),
               size_code=int(rng.choice([0, {8: 1, 16: 4, 24: 6}[bits]])))
    if rng.random() < 0.3 and code not in (6, 7):
        hdr["bs_code"] = 6 if bs <= 256 and rng.random() < 0.5 else 7
    fr = F.make_frame(rng, number, bs, bits, channels, assign, [m[0] for m in made], **hdr)
    hdr_len = R.header(fr[0], 0, bits)["headerLength"]
    fields = _fields(hdr_len, made[0][0], bits + (1 if side[0] else 0), bs)
    return fr, fields, {m[2] for m in made}, set().union(*[m[3] for m in made])


# ---------------------------------------------------------------------------------------------------------------- files

SPECIAL_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 192)


def _size(rng):
    p = rng.random()
    if p < 0.55:
        return int(rng.choice(SPECIAL_SIZES))
    if p < 0.75:
        return 2 * int(rng.integers(1, 256)) + 1
    if p < 0.85:
        return int(rng.choice([256, 512, 576]))
    return 2 * int(rng.integers(1, 257))


def _assemble(parts, frames=None, total=None):
    p = parts
    return F.flac_file(p["rate"], p["channels"], p["bits"], p["frames"] if frames is None else frames,
                       p["total"] if total is None else total, p["extra"], p["prefix"], p["trailer"])


def _build(name, rng, bits, channels, sizes, variable, cheap=False, decorate=True):
    frames, fields, numbers, types, runs, sample = [], [], [], set(), set(), 0
    for k, bs in enumerate(sizes):
        number = sample if variable else k
        fr, fl, ty, ru = _frame(rng, number, bs, bits, channels, variable, cheap)
        frames.append(fr)
        fields.append(fl)
        numbers.append(number)
        types |= ty
        runs |= ru
        sample += bs
    extra, prefix, trailer = [], b"", b""
    if decorate:
        if rng.random() < 0.3:
            extra = [[(1, bytes(int(rng.integers(0, 40)))), (4, struct.pack("<I", 3) + b"dcs" + struct.pack("<I", 0)), (3, bytes(18 * 2)),
                      (2, b"test" + bytes(8))][int(j)] for j in rng.integers(0, 4, int(rng.integers(1, 4)))]
        if rng.random() < 0.15:
            n = int(rng.integers(0, 300))
            prefix = b"ID3\x03\x00\x00" + bytes([0, 0, n >> 7, n & 0x7F]) + bytes(n)
        if rng.random() < 0.15:
            trailer = bytes(int(rng.integers(1, 200))) if rng.random() < 0.5 else b"TAG" + bytes(125)
    rate = int(rng.choice([8000, 11025, 22050, 31250, 44100, 48000, 96000]))
    parts = dict(rate=rate, channels=channels, bits=bits, frames=frames, total=sample, extra=extra, prefix=prefix, trailer=trailer,
                 fields=fields, numbers=numbers)
    data, ints = _assemble(parts)
    ints = np.asarray(ints, np.int64)
    ints.setflags(write=False)
    return Case(name, data, ints, (rate, channels, bits), frozenset(types), frozenset(runs), parts)


def _random_file(i):
    rng = np.random.default_rng([SEED, 1, i])
    bits, channels = (8, 16, 24)[i % 3], 1 + (i // 3) % 2
    variable = bool(rng.random() < 0.5)
    n = int(rng.integers(1, 5))
    if variable:
        sizes = [_size(rng) for _ in range(n)]
    else:
        bs = _size(rng)
        sizes = [bs] * n
        if rng.random() < 0.5 and bs > 1:
            sizes.append(int(rng.integers(1, bs)))             # a short last block
    return _build("random%03d_s%d_%dch" % (i, bits, channels), rng, bits, channels, sizes, variable)


def _sweep_files():
    """a unary run of `span` bits begun at each of 32 consecutive bit positions (and so ended at each of 32): fixed order 0,
    Rice parameter 0, p one-bit residuals in front of the run; eight frames a file"""
    out = []
    for si, span in enumerate((41, 64, 65, 96, 128, 129, 192)):
        for g in range(4):
            i = 4 * si + g
            bits, channels = (8, 16, 24)[i % 3], 1 + (i // 3) % 2
            rng = np.random.default_rng([SEED, 3, i])
            frames = []
            for p in range(8 * g, 8 * g + 8):
                specs, chans = [], []
                for c in range(channels):
                    u = [0] * p + [span - 1] + [int(x) for x in rng.integers(0, 3, 48 - p - 1)]
                    res = [(x >> 1) ^ -(x & 1) for x in u]
                    specs.append(F.S("fixed", order=0, k=0, exact=([], [], res)))
                    chans.append(res)
                frames.append(F.make_frame(rng, len(frames), 48, bits, channels, 0 if channels == 1 else 1, specs))
            parts = dict(rate=31250, channels=channels, bits=bits, frames=frames, total=48 * 8, extra=[], prefix=b"", trailer=b"",
                         fields=[_fields(R.header(f[0], 0, bits)["headerLength"], F.S("fixed", k=0), bits, 48) for f in frames],
                         numbers=list(range(8)))
            data, ints = _assemble(parts)
            out.append(Case("sweep_run%d_%d_s%d_%dch" % (span, g, bits, channels), data, np.asarray(ints, np.int64), (31250, channels, bits),
                            frozenset(["fixed0"]), frozenset([_run_class(span)]), parts))
    return out


def _shaped_files():
    """the remaining size codes and the number widths: cheap subframes, since the writer and the restatement are pure Python"""
    out = []
    shapes = [("sizes_576_family", 16, 1, [576, 1152, 2304, 4608, 100], True), ("sizes_pow2_small", 16, 2, [256, 512, 1024, 2048, 7], True),
              ("sizes_pow2_large", 8, 1, [4096, 8192, 16384, 32768, 3], True), ("sample_number_4_bytes", 16, 1, [32768, 32768, 17, 33], True),
              ("sample_number_3_bytes", 24, 2, [1152, 1152, 15, 1], True), ("frame_number_2_bytes", 16, 2, [2] * 140 + [1], False),
              ("frame_number_3_bytes", 8, 1, [1] * 2100, False), ("fixed_odd_37", 24, 1, [37] * 4 + [5], False),
              ("fixed_4608_short_last", 24, 1, [4608, 4608, 4607], False)]
    for j, (name, bits, channels, sizes, variable) in enumerate(shapes):
        out.append(_build(name, np.random.default_rng([SEED, 4, j]), bits, channels, sizes, variable, cheap=True, decorate=False))
    return out


@functools.lru_cache(maxsize=None)
def well_formed():
    return [_random_file(i) for i in range(N_RANDOM)] + _sweep_files() + _shaped_files()


# -------------------------------------------------------------------------------------------------------------- damage

MUTATIONS = ("flip_subframe_header", "flip_lpc_parameters", "flip_lpc_shift", "flip_partition_header", "flip_residual", "flip_residual", "truncate",
             "extend", "frame_number", "total_minus_block", "total_plus_block", "flip_residual_keep_crc", "flip_partition_header_keep_crc")


def _reframe(body):
    return body + struct.pack(">H", F.crc16(body))


def _flip(rng, frame, first, width):
    b = bytearray(frame[:-2])
    last = 8 * len(b)
    width = last - first if width is None else width
    if first >= last or width <= 0:
        return None
    for at in sorted(set(int(x) for x in rng.integers(first, min(last, first + width), int(rng.integers(1, 3))))):
        b[at >> 3] ^= 0x80 >> (at & 7)
    return bytes(b)


def _damage(j, pool):
    rng = np.random.default_rng([SEED, 2, j])
    mutation = MUTATIONS[j % len(MUTATIONS)]
    for _ in range(20):
        src = pool[int(rng.integers(len(pool)))]
        case = well_formed()[src]
        p = case.parts
        frames = list(p["frames"])
        f = int(rng.integers(len(frames)))
        old, chans = frames[f]
        total, body, fixed = None, None, not mutation.endswith("_keep_crc")
        if mutation.startswith("flip_"):
            field = mutation[5:].replace("_keep_crc", "")
            if field not in p["fields"][f]:
                continue
            body = _flip(rng, old, *p["fields"][f][field])
        elif mutation == "truncate":
            body = old[:-3] if len(old) > 12 else None
        elif mutation == "extend":
            body = old[:-2] + bytes([int(rng.choice([0, 0, 0xFF, int(rng.integers(256))]))])
        elif mutation == "frame_number":
            n = p["numbers"][f]
            cut = 4 + len(F.utf8(n))
            hl = R.header(old, 0, p["bits"])["headerLength"]
            h = old[:4] + F.utf8(n + int(rng.choice([1, 2, len(chans[0])]))) + old[cut:hl - 1]
            body = h + bytes([F.crc8(h)]) + old[hl:-2]
        else:
            bs = len(frames[-1][1][0])
            total = p["total"] + (bs if mutation == "total_plus_block" else -bs)
            if total <= 0:
                continue
        if total is None:
            if body is None:
                continue
            frames[f] = ((_reframe(body) if fixed else body + old[-2:]), chans)
        data = _assemble(p, frames, total)[0]
        if data != case.data:
            return Damaged("damaged%03d_%s_of_%s" % (j, mutation, case.name), data, src, mutation, fixed)
    raise AssertionError("no file takes mutation %s" % mutation)


@functools.lru_cache(maxsize=None)
def damaged():
    pool = [i for i, c in enumerate(well_formed()) if len(c.data) <= 6000 and len(c.parts["frames"]) <= 8]
    return [_damage(j, pool) for j in range(N_DAMAGED)]


# ----------------------------------------------------------------------------------------------------------- batches

def compositions(n, seed, alone=4):
    """the three ways a GPU test runs a set of n files: [("as generated", order, fillers)], order: indices into the set,
    fillers[i]: how many filler files (of 1 to 3 bytes' difference in length) go in front of the i-th of them; then a shuffle
    with fillers, then `alone` single files"""
    rng = np.random.default_rng([SEED, 5, seed])
    out = [("as generated", list(range(n)), [0] * n)]
    out.append(("shuffled with fillers", [int(x) for x in rng.permutation(n)], [int(x) for x in rng.integers(0, 3, n)]))
    for i in rng.choice(n, min(alone, n), replace=False):
        out.append(("alone %d" % i, [int(i)], [0]))
    return out


@functools.lru_cache(maxsize=None)
def fillers():
    """three small mono files whose lengths differ by 1 to 3 bytes modulo 4 (verbatim 8-bit blocks of 5, 6 and 7 samples)"""
    out = []
    for n in (5, 6, 7):
        rng = np.random.default_rng([SEED, 6, n])
        out.append(F.simple(int(rng.integers(1 << 30)), 8000, 1, 8, [(n, 0, [F.S("verbatim")])])[0])
    assert len({len(b) % 4 for b in out}) == 3
    return out


# ---------------------------------------------------------------------------------------------------------- the checker

def checker_available():
    return os.path.exists(EXE) and os.path.exists(EXE_SAN)


def _run_load(exe, files, tmp):
    pack, out = os.path.join(tmp, "pack.bin"), os.path.join(tmp, "out.bin")
    with open(pack, "wb") as f:
        f.write(struct.pack("<I", len(files)))
        for b in files:
            f.write(struct.pack("<Q", len(b)) + b)
    subprocess.run([exe, "load", pack, out, tmp], check=True, stdout=subprocess.DEVNULL, timeout=1200)
    raw, at, res = open(out, "rb").read(), 0, []
    for _ in files:
        kind, a, rate, _, n, m = struct.unpack_from("<iiiiQQ", raw, at)       # (the driver's struct Head, 4 bytes of padding)
        at += struct.calcsize("<iiiiQQ")
        size = 4 * n if kind == 0 else n if kind == 1 else 0
        payload, err = raw[at:at + size], raw[at + size:at + size + m].decode(errors="replace")
        at += size + m
        res.append((kind, a, rate, n, payload, err))
    assert at == len(raw)
    return res


def check_load(files):
    """NyquistIO::Load on every file, in the plain and in the sanitizer build -> [Load]: kind 'loaded' (channels, rate, count,
    sha256 of the float bits, the bits up to KEEP_VALUES), 'threw' (text) or 'crashed' (text: the wait status); reports: the
    sanitizer build's `runtime error` lines but VALUE_SHIFT's, or ['crashed'] / ['differs'] where that build alone crashed or answered otherwise"""
    files = [bytes(b) for b in files]
    with tempfile.TemporaryDirectory() as tmp:
        plain, san = _run_load(EXE, files, tmp), _run_load(EXE_SAN, files, tmp)
    out = []
    for (kind, a, rate, n, payload, _), s in zip(plain, san):
        said = {l.split("runtime error:")[1].strip() for l in s[5].splitlines() if "runtime error:" in l}
        reports = sorted(r for r in said if not VALUE_SHIFT.match(r))
        shifts = len(said) - len(reports)
        if not reports and s[0] != kind:
            reports = ["crashed" if s[0] == 2 else "differs"]
        elif not reports and s[4] != payload:
            reports = ["differs"]
        if kind == 0:
            out.append(Load("loaded", a, rate, n, hashlib.sha256(payload).hexdigest(),
                            np.frombuffer(payload, "<f4") if n <= KEEP_VALUES else None, None, reports, shifts))
        elif kind == 1:
            out.append(Load("threw", 0, 0, 0, None, None, payload.decode(errors="replace"), reports, shifts))
        else:
            out.append(Load("crashed", 0, 0, 0, None, None, "wait status %d" % a, reports, shifts))
    return out


def check_md5(pairs):
    """FLAC__stream_decoder with MD5 checking over (FLAC bytes, int16 source) pairs -> one verdict per pair, 'ok' or what failed"""
    with tempfile.TemporaryDirectory() as tmp:
        pack = os.path.join(tmp, "pack.bin")
        with open(pack, "wb") as f:
            f.write(struct.pack("<I", len(pairs)))
            for b, p in pairs:
                p = np.ascontiguousarray(p, "<i2").ravel()
                f.write(struct.pack("<QQ", len(b), p.size) + b + p.tobytes())
        run = subprocess.run([EXE, "md5", pack], stdout=subprocess.PIPE, universal_newlines=True, timeout=1200)
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(pairs) and run.returncode in (0, 1), (run.returncode, len(lines))
    return [l.split(" ", 1)[1] for l in lines]


# ------------------------------------------------------------------------------------------------------ the prediction

CODES = ("parse", "length", "depth", "shift")           # the device's kFlacErr* 1..4


def predict(b):
    """what flac_ref says the library does with a file -> dict(status, where: None / 'host' (dcs_flac_parse refuses) / 'device'
    (a kernel does), code: one of CODES for a device refusal, frame, reason).  The device reports the first frame at fault, and
    of that frame the walk's code before the restore's."""
    b = bytes(b)
    try:
        d, frames = R._read(b)
    except R.Refused as e:
        m = re.match(r"frame (\d+):", str(e))
        return dict(status=e.status, where="host", code=None, frame=int(m.group(1)) if m else None, reason=str(e))
    for i, f in enumerate(frames):
        h = R.header(b, f["offset"], d["bitDepth"])
        code = why = None
        try:
            subs, used = R.walk(b, f["offset"], f["offset"] + f["length"] - 2, h)
            if h["headerLength"] + used + 2 != f["length"]:
                code, why = "length", "a frame's parsed length differs from its indexed length"
            else:
                for s in subs:
                    R.restore(s)
        except R.Refused as e:
            why = str(e)
            code = "shift" if "shift" in why else "length" if "padding" in why else "depth" if "depth" in why else "parse"
            if "read past" in why:                          # would libFLAC, which knows no frame lengths, run out of file too?
                try:
                    R.walk(b, f["offset"], len(b), h)
                except R.Refused as e2:
                    why += " and past the file's end" if "read past" in str(e2) else ""
        if code:
            return dict(status=R.BAD_STREAM, where="device", code=code, frame=i, reason=why)
    return dict(status=R.OK, where=None, code=None, frame=None, reason="")


def stricter_clause(p):
    """the clause of INTEGRATION.md "Encoding files" rules 20-25 under which the library refuses a file that libFLAC decodes,
    or None: frame numbers (libFLAC does not compare them; with every CRC right by libFLAC's own check, an index that finds no
    confirming candidate can only have passed over a wrongly numbered one), a sample outside its depth, padding, length, a negative
    LPC shift, a partition order that does not fit the block; and the
    two this fuzz added to rule 23: the file ends inside a frame as libFLAC reads it (it ends the stream there without a word,
    and the reference keeps zeros from that frame on; on the host flac_ref raises these three reasons only for the frame that
    completes the total, which it reads up to the file's end), and wasted bits that leave no bit of the sample"""
    r = p["reason"]
    if "wasted" in r:
        return "wasted bits"
    if "negative LPC shift" in r:
        return "negative LPC shift"
    if "partition order" in r:
        return "partition order"
    if "read past" in r and (p["where"] == "host" or "past the file's end" in r) or "CRC-16" in r or "padding" in r and p["where"] == "host":
        return "end of file inside a frame"
    if p["where"] == "host":
        if "number" in r or "no candidate confirms" in r:
            return "frame numbers"
        if "more samples than STREAMINFO" in r or "lost sync" in r:
            return "length"
        return None
    return {"depth": "sample outside its depth", "length": "padding" if "padding" in r else "length"}.get(p["code"])


# ------------------------------------------------------------------------------------- the pack for the sanitizer program

def walk_pack():
    """every file the GPU tests upload: flac_cases' accepted and refused cases, the well-formed and the damaged files, the fillers"""
    return ([b for _, b in F.cases()] + [c[1] for c in F.refused_cases()] + [c.data for c in well_formed()]
            + [d.data for d in damaged()] + list(fillers()))


def main(argv):
    """python tests/flac_fuzz_cases.py --pack FILE: FILE for tests/cpp/dcs_flac_walk_san.cpp, and FILE.expect with what flac_ref
    predicts for each file, in the first three fields of that program's lines"""
    if len(argv) != 3 or argv[1] != "--pack":
        sys.stderr.write(main.__doc__ + "\n")
        return 2
    files = walk_pack()
    with open(argv[2], "wb") as f:
        f.write(struct.pack("<I", len(files)))
        for b in files:
            f.write(struct.pack("<Q", len(b)) + b)
    with open(argv[2] + ".expect", "w") as f:
        for i, b in enumerate(files):
            p = predict(b)
            err = "%d:%d" % (p["frame"], 1 + CODES.index(p["code"])) if p["where"] == "device" else "-"
            f.write("%d %d %s\n" % (i, p["status"] if p["where"] == "host" else 0, err))
    print("%d files in %s" % (len(files), argv[2]))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main(sys.argv))
