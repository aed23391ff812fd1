"""Seeded DCS streams for the fuzz of the decoder against the compiled reference decoder (tests/test_decode_vs_reference.py,
tests/test_gpu_decode_vs_reference.py), and the compiled checker itself (test infrastructure).  Every case is a recipe: seeds
that produce bytes through dcs_synth_stream or through the bit writer below; no stream bytes are committed.

A case is Case(name, os, volume, chans, extra_frames, cls, tags): chans = [(level, bytes)], the streams loaded at tick 0 on
channels 0 .. n-1 of a fresh decoder; frames pulled = the largest frame count among them + extra_frames.  Streams have 3 to
40 frames (a damaged one may claim up to 8 more).

  reheaded() -> R  dcs_synth_stream output of the five layouts with a 16-byte header, every profile, 1 .. 16 header bands, with
                   the low six bits of every header byte before the terminator redrawn in 0 .. 63 (bits 6 and 7 kept, no byte
                   made a terminator); 1994+: every second case has its two sub-format bits set to each of the four values in
                   turn, on Type 0 and on Type 1.  OS93a Type 1 has no such header: profile 3 with 1 .. 18 bands.
  written()  -> W  1994+ streams written from the decoder's side by write94(): strided bands as any subset, the terminator at
                   every band 0 .. 16, scale codes 0 .. 63, band-type deltas of -16 and +14, every entry of every sample
                   codebook, a two-zeros code as a band's last pair and with one sample left (a stop without fatal), fixed
                   widths 7 .. 16 at their two extremes.  tags: "stop" / "fatal" where the recipe asks for that flag.
  damaged()  -> D  payload flips, drawn and aimed (a code turned into its book's two-zeros code); header flips from byte 2 on; random
                   bytes after the header; cut mid-frame, bare and with zero padding; the frame count raised with zero padding behind -- of R and W streams.
  mixes()    -> M  2 .. 8 clean R / W streams of one OS version on one decoder, lengths and levels differing.
  past_the_row(n)  the smallest streams that showed a fault of the library's: OS93 Type 0 frames that leave their 256 words
  lists()          the single-stream cases dealt into lists of 24 to 48 for the GPU: lists of 1994+ streams only (the kernels
                   of single-source 1994+ batches) and lists of both families, the classes shuffled together in each

flags(oracle, case) is what the restatement says of a case (per channel: the stop words of all its frames), fatal() / stopped()
the screens made from it.  The reference indexes a table with whatever band-type code a damaged stream leaves, so a case with a
fatal flag in ANY frame is one the reference does not define (its GetStreamInfo walks every frame, stopped or not).  overruns()
is the second screen: OS93 Type 0 headers whose frames reach behind the reference's frame buffer.  undefined() is either.

run_reference() runs oracle/_ref/dcs_decref or dcs_decref_san (`make -C oracle decref`) over cases, a child process a case."""
import collections
import functools
import os
import re
import struct
import subprocess
import tempfile

import numpy as np

import dcsexplorer_amd as D
import enc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
EXE, EXE_SAN = os.path.join(REF_DIR, "dcs_decref"), os.path.join(REF_DIR, "dcs_decref_san")
MISSING = "oracle/_ref/dcs_decref* not built (needs the reference sources; `make -C oracle decref`)"
SEED = 0xDEC0DE

Case = collections.namedtuple("Case", "name os volume chans extra_frames cls tags")
Ref = collections.namedtuple("Ref", "kind status pcm infos stderr")

FORMATS_94 = (D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3)
LAYOUTS_16 = (D.FMT_93_T0, D.FMT_93B_T1) + FORMATS_94
FORCED_VOLUMES, FORCED_LEVELS = (0, 1, 127, 255), (0, 1, 127)


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def n_frames(stream):
    return (stream[0] << 8) | stream[1]


def _volume_level(rng, k):
    """0, 1, 127 and 255 forced in at the start of a class, then drawn over 0 .. 255 and 0 .. 127"""
    vol = FORCED_VOLUMES[k % 4] if k < 8 else int(rng.integers(256))
    lvl = FORCED_LEVELS[(k // 4) % 3] if 4 <= k < 16 else int(rng.integers(128))
    return vol, lvl


# ------------------------------------------------------------------------------------------------------------ R: re-headed

def rehead(stream, rng, sub=None):
    """the low six bits of every header byte before the terminator redrawn; sub: the two sub-format bits (1994+), or None"""
    b = bytearray(stream)
    for i in range(2, 18):
        if b[i] & 0x7F == 0x7F:
            break
        while True:
            v = (b[i] & 0xC0) | int(rng.integers(64))
            if v & 0x7F != 0x7F:
                break
        b[i] = v
    if sub is not None:
        b[3] = (b[3] & 0x7F) | ((sub & 2) << 6)
        b[4] = (b[4] & 0x7F) | ((sub & 1) << 7)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def reheaded():
    out = []
    for li, fmt in enumerate(LAYOUTS_16):
        is94 = fmt in FORMATS_94
        profiles = 6 if is94 else 7
        for k in range(44):
            rng = _rng(1, li, k)
            nbands, profile = 1 + k % 16, k % profiles
            stride_from = (16, max(nbands // 2, 1), 2, max(nbands - 1, 1))[(k // 4) % 4]
            s = D.synth_stream(fmt, 3 + int(rng.integers(38)), 7000 + 100 * li + k, nbands=nbands, stride_from=stride_from, profile=profile)
            sub = (k // 2) % 4 if is94 and k % 2 else None
            vol, lvl = _volume_level(rng, len(out))
            os_ = D.api.format_os(fmt, prefer_95=bool(k & 1), prefer_93a=bool(k & 1))
            name = "R%03d_f%d_p%d_b%d_s%d%s" % (len(out), fmt, profile, nbands, stride_from, "" if sub is None else "_sub%d" % sub)
            out.append(Case(name, os_, vol, ((lvl, rehead(s, rng, sub)),), int(rng.integers(3)), "R", frozenset()))
    for nbands in range(1, 19):
        rng = _rng(1, 9, nbands)
        s = D.synth_stream(D.FMT_93A_T1, 3 + int(rng.integers(38)), 7900 + nbands, nbands=nbands, profile=3)
        vol, lvl = _volume_level(rng, len(out))
        out.append(Case("R%03d_93a_b%d" % (len(out), nbands), D.OS93A, vol, ((lvl, s),), int(rng.integers(3)), "R", frozenset()))
    return out


# ------------------------------------------------------------------------- W: 1994+ streams written from the decoder's side

class Bits:
    """MSB first, zero-padded to a byte"""
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, n):
        assert 0 <= value < (1 << n) and n > 0
        self.acc, self.n = (self.acc << n) | value, self.n + n

    def bytes(self):
        pad = -self.n % 8
        return ((self.acc << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


BAND_COUNT = [int(x) for x in enc_ref.BAND_COUNT]
for _w in range(1, 7):
    assert (enc_ref.SMP_LEN[_w] > 0).all() and enc_ref.DZ_LEN[_w] > 0          # (every index and the two-zeros code have a code)
assert (enc_ref.HDR_LEN > 0).all()                                              # (deltas -16 .. +14)
DZ = "two zeros"
BOOK_ENTRIES = {w: list(range(1 << w)) + [DZ] for w in range(1, 7)}


def width_of(typ, band, code):
    """the sample code of a band-type code: Type 0 is the width itself, Type 1 goes through the band group's table"""
    return code if typ == 0 else int(enc_ref.XLAT[0 if band < 3 else 1 if band < 6 else 2][code]) & 0xFF


def _code_of_width(typ, band, want, rng):
    """a band-type code (1 ..) whose samples have width `want`, else one of the nearest width the layout has"""
    codes = range(1, 17 if typ == 0 else 16)
    best = min(abs(width_of(typ, band, c) - want) for c in codes)
    pick = [c for c in codes if abs(width_of(typ, band, c) - want) == best]
    return pick[int(rng.integers(len(pick)))]


def write94(rng, mode, typ, sub, term, frames, arg=0, log=None, marks=None):
    """one 1994+ stream: `term` header bands (the terminator stands at byte `term`; what lies behind it is drawn), Type `typ`,
    sub-format bits `sub`.  mode:
      "random"   codes kept with 70 % or drawn over the layout's range, samples drawn over every entry of the band's codebook
      "books"    every band's width cycles 1 .. 6 and the samples run through every entry of the codebooks in turn
      "ends"     Type 0: codes 14, 16, 0, ... (deltas +14, +2, -16); Type 1: 0 / 14 and 1 / 15 (deltas +14, -14)
      "under"    Type 1: as random, and in the last frame band `arg`'s delta is -16 from a code below 16: fatal
      "dz_last"  widths 1 .. 6, every band ends in a two-zeros code
      "dz_one"   as dz_last, but in frame `arg` one band has the two-zeros code with one sample left: a stop without fatal
      "fixed"    Type 0: every band at width `arg` (7 .. 16), samples -2^(w-1) and 2^(w-1)-1 in turn with drawn ones between;
                 Type 1: the widest codes of each band group (widths 7 and 8)
      "scale"    as random with codes of 5 and more, header scale codes (16 * arg + band) % 64 and, Type 1, 48 .. 63 in odd bands
    log: dict collecting "entries" {(width, entry)}, "deltas" {delta}, "fixed" {(width, value)}
    marks: list collecting (payload bit, width, entry, samples left) of every one-sample code in a band that ends in a two-zeros pair"""
    log = {} if log is None else log
    entries, deltas, fixed = log.setdefault("entries", set()), log.setdefault("deltas", set()), log.setdefault("fixed", set())
    max_code = 15 if typ else 16
    hdr = bytearray(rng.integers(0, 256, 16).astype(np.uint8).tobytes())
    strided = [False] * 16
    for b in range(term):
        sc = int(rng.integers(64))
        if mode == "scale":
            sc = (16 * arg + b) % 64 if not (typ and b & 1) else 48 + int(rng.integers(16))
        strided[b] = bool(rng.integers(2)) and sc != 63                # (63 with the stride bit is a terminator)
        hdr[b] = sc | (0x40 if strided[b] else 0)
    if term < 16:
        hdr[term] |= 0x7F
    hdr[0] = (hdr[0] & 0x7F) | (typ << 7)
    hdr[1] = (hdr[1] & 0x7F) | ((sub & 2) << 6)
    hdr[2] = (hdr[2] & 0x7F) | ((sub & 1) << 7)
    w = Bits()
    code = [0] * 16
    at = {k: 0 for k in range(1, 7)}                                    # "books": where each codebook's run stands
    stop_band = int(rng.integers(term)) if mode == "dz_one" and term else -1
    for f in range(frames):
        last = f == frames - 1
        for b in range(term):
            if mode == "books" or mode in ("dz_last", "dz_one"):
                target = _code_of_width(typ, b, 1 + (b + f) % 6, rng)
            elif mode == "ends":
                target = ((14, 16, 0)[(f + b) % 3] if typ == 0 else (0, 14)[(f + b // 2) % 2] + (b & 1))
            elif mode == "fixed":
                target = arg if typ == 0 else (13 + (f + b) % 3 if b < 3 else 15)
            elif f == 0 or rng.random() >= 0.7:
                target = int(rng.integers(5 if mode == "scale" else 0, max_code + 1))
            else:
                target = code[b]
            delta = max(-16, min(14, target - code[b]))
            if mode == "under" and last and b == arg:
                delta = -16
            code[b] += delta
            deltas.add(delta)
            w.put(int(enc_ref.HDR_CODE[delta + 16]), int(enc_ref.HDR_LEN[delta + 16]))
        if mode == "under" and last:
            assert code[arg] < 0                                        # (the reference's uint16 wraps: a code above 15)
            break
        for b in range(term):
            if code[b] == 0:
                continue
            width = width_of(typ, b, code[b])
            count = BAND_COUNT[b] >> strided[b]
            if width > 6:
                lo, hi = -(1 << (width - 1)), (1 << (width - 1)) - 1
                for i in range(count):
                    v = (lo, hi)[(i // 2) & 1] if mode == "fixed" and i % 2 == 0 else int(rng.integers(lo, hi + 1))
                    fixed.add((width, v))
                    w.put(v & ((1 << width) - 1), width)
                continue
            i = count
            ends_in_pair = mode == "dz_last" or (mode == "dz_one" and not (f == arg and b == stop_band))
            while i > 0:
                if mode == "books":
                    e = BOOK_ENTRIES[width][at[width] % len(BOOK_ENTRIES[width])]
                    if e is DZ and i < 2:
                        e = int(rng.integers(1 << width))
                    else:
                        at[width] += 1
                elif mode in ("dz_last", "dz_one") and i == 2 and not (mode == "dz_one" and f == arg and b == stop_band):
                    e = DZ
                elif mode == "dz_one" and f == arg and b == stop_band and i == 1:
                    e = DZ                                              # one sample left: the stop
                elif i >= 2 and mode not in ("dz_last", "dz_one") and rng.random() < 0.12:
                    e = DZ
                else:
                    e = int(rng.integers(1 << width))
                entries.add((width, e))
                if e is DZ:
                    w.put(int(enc_ref.DZ_CODE[width]), int(enc_ref.DZ_LEN[width]))
                    i -= 2
                else:
                    if marks is not None and ends_in_pair:
                        marks.append((w.n, width, e, i))
                    w.put(int(enc_ref.SMP_CODE[width][e]), int(enc_ref.SMP_LEN[width][e]))
                    i -= 1
    return bytes([frames >> 8, frames & 0xFF]) + bytes(hdr) + w.bytes()


def _w_recipes():
    """(mode, typ, sub, term, arg, tags) of every W case"""
    out = []
    for term in range(17):                                              # the terminator at every band, both types
        for typ in (0, 1):
            out.append(("random", typ, (term + 2 * typ) % 4, term, 0, ()))
    for k in range(24):                                                 # every entry of every codebook
        out.append(("books", (0, 1, 1)[k % 3], k % 4, 16 - k % 5, 0, ()))
    for k in range(8):
        out.append(("ends", 0, k % 4, 16 - k, 0, ()))
    for k in range(4):
        out.append(("ends", 1, k, 16 - 3 * k, 0, ()))
    for k in range(4):
        out.append(("under", 1, k, 16 - 2 * k, (0, 2, 5, 9)[k], ("fatal",)))
    for k in range(10):
        out.append(("dz_last", k % 2, k % 4, 16 - k, 0, ()))
    for k in range(10):
        out.append(("dz_one", k % 2, (k + 1) % 4, 16 - k % 7, 1 + k % 2, ("stop",)))
    for width in range(7, 17):
        out.append(("fixed", 0, width % 4, 16 if width < 15 else 12, width, ()))
    out += [("fixed", 1, 0, 16, 0, ()), ("fixed", 1, 3, 11, 0, ())]
    for k in range(12):
        out.append(("scale", (1, 1, 0)[k % 3], k % 4, 16 - k % 4, k % 4, ()))
    return out


W_LOG = {}
W_MARKS = {}                    # name of a "dz_last" case -> write94's marks


@functools.lru_cache(maxsize=None)
def written():
    out = []
    for k, (mode, typ, sub, term, arg, tags) in enumerate(_w_recipes()):
        rng = _rng(2, k)
        frames = 3 + int(rng.integers(38))
        if mode in ("books", "fixed", "ends"):
            frames = max(frames, 8)
        name = "W%03d_%s_t%d_sub%d_term%d" % (k, mode, typ, sub, term)
        s = write94(rng, mode, typ, sub, term, frames, arg, W_LOG, W_MARKS.setdefault(name, []) if mode == "dz_last" else None)
        vol, lvl = _volume_level(rng, k)
        out.append(Case(name, D.OS95 if k & 1 else D.OS94, vol, ((lvl, s),), int(rng.integers(3)), "W", frozenset(tags)))
    return out


# ------------------------------------------------------------------------------------------------------------- D: damaged

# (how many of each: bytes that run out into zeros -- a cut, a raised count -- or into noise end a 1994+ stream in a band-type
# code no table has, which is fatal, within a frame or two: the delta code of two zero bits is -1.  A stop WITHOUT fatal is one
# event only, a two-zeros code with one sample of its band left, and random flips make it in a few streams in a hundred; the
# aimed flips make it on purpose.)
MUTATIONS = (("payload_flips", 90), ("aimed_flip", 60), ("header_flips", 90), ("random_payload", 24), ("cut_bare", 24), ("cut_padded", 24),
             ("count_raised", 48))
N_DAMAGED = sum(n for _, n in MUTATIONS)


def _flip(b, rng, first, n):
    for _ in range(n):
        at = first + int(rng.integers(max(1, len(b) - first)))
        if at < len(b):
            b[at] ^= 1 << int(rng.integers(8))


def damage(case, mutation, rng):
    lvl, s = case.chans[0]
    hdr_end = 2 + (1 if case.os == D.OS93A and s[2] & 0x80 else 16)
    b = bytearray(s)
    if mutation == "payload_flips":
        _flip(b, rng, hdr_end, 1 + int(rng.integers(3)))
        b += bytes(256)
    elif mutation == "aimed_flip":
        # one payload bit: a one-sample code that is one bit away from its book's two-zeros code, in a band that ends in a two-zeros
        # pair, becomes that code; the band's last code then comes with one sample left, and every later code stands where it stood
        aims = []
        for at, width, e, left in W_MARKS[case.name]:
            code, n = int(enc_ref.SMP_CODE[width][e]), int(enc_ref.SMP_LEN[width][e])
            diff = code ^ int(enc_ref.DZ_CODE[width])
            if n == int(enc_ref.DZ_LEN[width]) and diff and diff & (diff - 1) == 0 and left >= 3:
                aims.append(at + n - diff.bit_length())
        at = aims[int(rng.integers(len(aims)))]
        b[hdr_end + (at >> 3)] ^= 0x80 >> (at & 7)
        b += bytes(256)
    elif mutation == "header_flips":                                    # one flip inside the header, up to three anywhere behind byte 2
        at = 2 + int(rng.integers(hdr_end - 2))
        b[at] ^= 1 << int(rng.integers(8))
        _flip(b, rng, 2, int(rng.integers(3)))
        b += bytes(256)
    elif mutation == "random_payload":
        b[hdr_end:] = rng.integers(0, 256, max(len(b) - hdr_end, 8)).astype(np.uint8).tobytes()
    elif mutation in ("cut_bare", "cut_padded"):
        pay = len(b) - hdr_end
        del b[hdr_end + pay // 4 + int(rng.integers(max(1, pay // 2))):]
        if mutation == "cut_padded":
            b += bytes(256)
    else:
        more = 1 + int(rng.integers(8))
        n = n_frames(s) + more
        b[0], b[1] = n >> 8, n & 0xFF
        b += bytes(1024 * more)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def damaged():
    pool = [c for c in reheaded() + written() if not c.tags]
    aimed = [c for c in written() if c.name in W_MARKS]
    kinds = [m for m, n in MUTATIONS for _ in range(n)]
    out = []
    for j in range(N_DAMAGED):
        rng = _rng(3, j)
        mutation = kinds[j]
        src = (aimed if mutation == "aimed_flip" else pool)[int(rng.integers(len(aimed if mutation == "aimed_flip" else pool)))]
        out.append(Case("D%03d_%s_of_%s" % (j, mutation, src.name), src.os, src.volume, ((src.chans[0][0], damage(src, mutation, rng)),),
                        int(rng.integers(3)), "D", frozenset([mutation])))
    return out


# --------------------------------------------------------------------------------------------------------------- M: mixes

@functools.lru_cache(maxsize=None)
def mixes():
    by_os = collections.defaultdict(list)
    for c in reheaded() + written():
        if not c.tags:
            by_os[c.os].append(c)
    out = []
    for j in range(40):
        rng = _rng(4, j)
        pool = by_os[(D.OS94, D.OS95, D.OS93B, D.OS93A)[j % 4]]
        n = 2 + j % 7
        picks = [pool[int(i)] for i in rng.choice(len(pool), n, replace=False)]
        chans = tuple((int(rng.integers(128)), c.chans[0][1]) for c in picks)
        out.append(Case("M%02d_os%d_x%d" % (j, picks[0].os, n), picks[0].os, (255, 200, 90, int(rng.integers(256)))[j % 4], chans, 1, "M", frozenset()))
    return out


def past_the_row(n_strided, frames=6, seed=0):
    """the smallest streams whose frames leave their 256 words: OS93 Type 0, the stride bit set in the header of the first
    `n_strided` bands (a strided band takes 32 words, the others 16; the payload parses as it did: Type 0 has sixteen samples a
    band either way).  Up to 15: a synthetic stream of fifteen bands (all strided: word 481).  16: sixteen strided bands over a
    drawn payload -- every bit pattern is a Type 0 frame, a band's code has four bits -- which reach word 513, where the output
    index no longer fits the record's nine bits and the reference writes behind its frame buffer"""
    if n_strided == 16:
        rng = _rng(6, seed)
        hdr = bytes(0x40 | int(x) for x in rng.integers(8, 40, 16))
        b = bytes([0, frames]) + hdr + rng.integers(0, 256, frames * 16 * 34).astype(np.uint8).tobytes()
    else:
        b = bytearray(D.synth_stream(D.FMT_93_T0, frames, 8100 + seed, nbands=15, stride_from=16, profile=0))
        assert all(b[2 + k] & 0x7F != 0x7F and not b[2 + k] & 0x40 for k in range(15)) and b[17] & 0x7F == 0x7F
        for k in range(n_strided):
            b[2 + k] |= 0x40
    return Case("past_the_row_%d" % n_strided, D.OS93B, 255, ((0x64, bytes(b)),), 1, "D", frozenset(["stride_bits"]))


def singles():
    return reheaded() + written() + damaged()


def is94(case):
    return case.os in (D.OS94, D.OS95)


@functools.lru_cache(maxsize=None)
def lists():
    """[(name, 1994+ only, [Case])]: the single-stream cases, shuffled, in lists of 24 to 48; two thirds of the 1994+ cases in
    lists of their own, the rest with the 1993 cases"""
    rng = _rng(5)
    new = [c for c in singles() if is94(c)]
    old = [c for c in singles() if not is94(c)]
    new = [new[int(i)] for i in rng.permutation(len(new))]
    cut = 2 * len(new) // 3
    out = []
    for only94, pool in ((True, new[:cut]), (False, old + new[cut:])):
        n_lists = -(-len(pool) // 36)
        dealt = [[] for _ in range(n_lists)]
        at = 0
        for cls in "RWD":                                               # every class dealt round, so that every list has all three
            members = [c for c in pool if c.cls == cls]
            for i in rng.permutation(len(members)):
                dealt[at % n_lists].append(members[int(i)])
                at += 1
        for l in dealt:
            out.append(("%s%02d" % ("new" if only94 else "both", len(out)), only94, [l[int(i)] for i in rng.permutation(len(l))]))
    return out


# ------------------------------------------------------------------------------------------ what the restatement says of a case

_FLAGS = {}


def flags(oracle, case):
    """per channel: the oracle's stop | fatal << 1 of every frame the stream claims (decompress walks on behind a stop, as the
    reference's GetStreamInfo does)"""
    if case.name not in _FLAGS:
        _FLAGS[case.name] = [oracle.decompress(case.os, s, 0x7FFF, n_frames(s))[3] for _, s in case.chans]
    return _FLAGS[case.name]


def fatal(oracle, case):
    return any(bool((st & 2).any()) for st in flags(oracle, case))


def stopped(oracle, case):
    """a stop without fatal anywhere, and no fatal flag"""
    return not fatal(oracle, case) and any(bool((st & 1).any()) for st in flags(oracle, case))


def overruns(case, words=512):
    """a stream of the case is OS93 Type 0 with so many strided bands (32 words each, 16 the others) that a frame's samples can
    reach word `words`.  512: the reference's decoder writes behind its frame buffer (INTEGRATION.md "Damaged streams", 3);
    256: its GetStreamInfo, which unpacks into 256 words, does.  The library drops what lies past word 255.  From the header
    alone: every band taken as coded."""
    if is94(case):
        return False
    for _, s in case.chans:
        if s[2] & 0x80:
            continue
        at = 1
        for k in range(16):
            if s[2 + k] & 0x7F == 0x7F:
                break
            at += 32 if s[2 + k] & 0x40 else 16
            if at > words:
                return True
    return False


def undefined(oracle, case):
    """the reference does not define the case's answer: a fatal flag, or samples behind its frame buffer"""
    return fatal(oracle, case) or overruns(case)


def frames_out(case):
    return max(n_frames(s) for _, s in case.chans) + case.extra_frames


def oracle_pcm(oracle, case):
    return oracle.decode(case.os, case.volume, [s for _, s in case.chans], [l for l, _ in case.chans], frames_out(case))


def band_stats(oracle, case):
    """of a single 1994+ stream, from the header and the oracle's band-type codes after every frame up to its first stop:
    [(type, band, header scale code, the sum the decoder makes of it (Type 1: + pre-adjust + the table's adjustment))] of
    every band with a code"""
    _, s = case.chans[0]
    hdr = s[2:18]
    typ = hdr[0] >> 7
    sub = ((hdr[1] & 0x80) >> 6) | ((hdr[2] & 0x80) >> 7)
    nb = next((i for i in range(16) if hdr[i] & 0x7F == 0x7F), 16)
    _, _, codes, stops = oracle.decompress(case.os, s, 0x7FFF, n_frames(s))
    out, prev = [], np.zeros(16, np.int64)
    for f in range(len(stops)):
        if stops[f] & 2:
            break
        for b in range(nb):
            c = int(codes[f, b])
            if c == 0:
                continue
            total = hdr[b] & 0x3F
            if typ:
                total += int(enc_ref.PREADJ[0 if sub == 0 else 3][prev[b]]) if b < 3 else 0
                total += int(enc_ref.XLAT[0 if b < 3 else 1 if b < 6 else 2][c]) >> 8
            out.append((typ, b, hdr[b] & 0x3F, total))
        if stops[f]:
            break
        prev = codes[f].astype(np.int64)
    return out


def header_facts(case):
    """(type, sub-format bits, header bands, the strided bands as a tuple of flags) of a single 1994+ stream"""
    hdr = case.chans[0][1][2:18]
    nb = next((i for i in range(16) if hdr[i] & 0x7F == 0x7F), 16)
    return hdr[0] >> 7, ((hdr[1] & 0x80) >> 6) | ((hdr[2] & 0x80) >> 7), nb, tuple(bool(hdr[i] & 0x40) for i in range(nb))


def is_suffix(strided):
    return list(strided) == sorted(strided)


# ------------------------------------------------------------------------------------------------------------ the checker

def checker_available():
    return os.path.exists(EXE) and os.path.exists(EXE_SAN)


def run_reference(cases, san=False):
    """-> [Ref]: kind "decoded" (status: 0, or -2 where the decoder's IsOK() is false; pcm int16 [frames, 240]; infos: per channel
    GetStreamInfo's dict -- None, and status the wait status, where the child crashed in GetStreamInfo with the PCM handed over) or
    "crashed" (status: the wait status); stderr: what the child wrote (the sanitizer build's reports)"""
    with tempfile.TemporaryDirectory() as tmp:
        pack, out = os.path.join(tmp, "pack.bin"), os.path.join(tmp, "out.bin")
        with open(pack, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for c in cases:
                f.write(struct.pack("<iiii", c.os, c.volume, len(c.chans), frames_out(c)))
                for lvl, s in c.chans:
                    f.write(struct.pack("<iQ", lvl, len(s)) + s)
        subprocess.run([EXE_SAN if san else EXE, "decode", pack, out], check=True, stdout=subprocess.DEVNULL, timeout=1200)
        raw = open(out, "rb").read()
    at, res = 0, []
    for c in cases:
        kind, status, nch, _, n, m = struct.unpack_from("<iiiiQQ", raw, at)
        at += struct.calcsize("<iiiiQQ")
        pcm, infos = None, None
        if kind in (0, 1):
            pcm = np.frombuffer(raw, "<i2", n, at).reshape(-1, 240)
            at += 2 * n
        if kind == 0:
            infos = []
            for _ in range(nch):
                nf, nb, ft, fs = struct.unpack_from("<iiii", raw, at)
                infos.append(dict(nFrames=nf, nBytes=nb, formatType=ft, formatSubType=fs, header=raw[at + 16:at + 32]))
                at += 32
        res.append(Ref("crashed" if kind == 2 else "decoded", status, pcm, infos, raw[at:at + m].decode(errors="replace")))
        at += m
    assert at == len(raw)
    return res


# The reference sign-extends and scales with `<<` on signed values in its transforms and in the OS93 unpack (DCSDecoderNative.cpp
# :2526, :3542-3577), on every stream there is.  ISO C++17 leaves a left shift of a negative value undefined; GCC, which builds the
# checker, defines it, and both builds give the same PCM.  And :2991 shifts by a count of 32 or more where a damaged OS93a stream
# drives a scale code out of its range: the library's masked-shift rule (INTEGRATION.md "Damaged streams", 4).  Both are counted
# and do not set a case aside; every other report does.
VALUE_SHIFT = re.compile(r"left shift of negative value -?\d+$")
MASKED_SHIFT = re.compile(r"DCSDecoderNative\.cpp:2991:\d+: runtime error: shift exponent \d+ is too large for 32-bit type 'unsigned int'$")


def reports(ref):
    """the sanitizer build's `runtime error` lines of one case -> (those that set it aside, value shifts, masked shifts)"""
    lines = {l.strip() for l in ref.stderr.splitlines() if "runtime error:" in l}
    value = {l for l in lines if VALUE_SHIFT.search(l)}
    masked = {l for l in lines if MASKED_SHIFT.search(l)}
    return sorted(l.split("runtime error:")[1].strip() for l in lines - value - masked), len(value), len(masked)
