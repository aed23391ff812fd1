"""Budgets from any source, restated from the restatements that exist: a WAV or FLAC file read
(wav_ref, flac_ref), any-rate PCM converted (resample_ref) and levelled (level_ref), an existing stream decoded as the
recipe plays it (transcode_ref.decoded, enc_ref.to_float), then the searched encoders (enc94rd_ref, enc93rd_ref) per job or
under one shared allocation (encrd_fit_ref).  What is stated here and nowhere else: the copy rule, and the copies' bytes
coming off a shared total before the searched jobs share what is left.  Also the small lists the host and GPU tests run."""
import functools
import hashlib

import numpy as np

import dcsexplorer_amd as D
import enc93rd_ref as R93
import enc94rd_ref as R94
import enc_ref as E
import encrd_fit_ref as FR
import flac_cases
import flac_ref
import level_ref
import resample_ref as RS
import transcode_ref as T
import wav_cases
import wav_ref
from util import make_stream

VERSIONS = [0x9400, 0x9302, 0x9301]
FMT94 = (0, 0)                  # the 1994+ layout the lists are searched in (one trellis a job keeps the restatement quick)
MQE = R94.DEFAULTS["maximumQuantizationError"]
OS_OF = {0x9400: D.OS94, 0x9302: D.OS93B, 0x9301: D.OS93A}
INFO_KEYS = ("formatType", "formatSubType", "ladderIndex", "numBands", "frameBits", "budgetBits", "sqErr", "fits")
COPY_INFO = (0, 0, 0, 0, 0, 0, 0, 1)


# ------------------------------------------------------------------------------------------------ the searched encoders

def analyse(x, version):
    return R94.analyse(x) if version == 0x9400 else R93.analyse(x, version)


def curve(an, version):
    return FR.curve94(R94, an, FMT94, MQE) if version == 0x9400 else FR.curve93(R93, an, MQE)


def encode(an, version, budget_bytes, rate=None):
    """-> (bytes, info tuple in INFO_KEYS' order, the restatement's own result); budget_bytes None: the rate's frame bits"""
    p = {} if rate is None else dict(targetBitRate=rate)
    r = R94.encode(an, FMT94, budget_bytes, **p) if version == 0x9400 else R93.encode(an, budget_bytes, **p)
    ch = r[1]
    return r[0], (ch["type"], ch["sub"], ch["ladderIndex"], ch["numBands"], ch["frameBits"], ch["budgetBits"], ch["sqErr"], int(ch["fits"])), r


# -------------------------------------------------------------------------------------------------------- the copy rule

def copied(copyable, length, j, budget=None, total=None, cap=None, reencode_all=False):
    """is job j, a source of `length` bytes that transcoding would copy (copyable), copied under the budget?"""
    if reencode_all or not copyable:
        return False
    most = cap if total is not None else budget
    return most is None or length <= most[j]


def run(version, units, budget=None, total=None, cap=None, rate=None):
    """units: per job ("copy", bytes) or ("pcm", float32 at 31 250 Hz).  Per job form (total None): searched job j to
    budget[j] bytes (budget None: the rate's bits).  Shared form: the copies are taken first, the searched jobs share
    max(total - copies, 0) under their own caps.  -> (streams, info tuples, record dict or None, allotments or None, per job
    None or (the restatement's own result, its analysis))"""
    n = len(units)
    searched = [j for j in range(n) if units[j][0] == "pcm"]
    ans = {j: analyse(units[j][1], version) for j in searched}
    streams, infos, raws = [None] * n, [COPY_INFO] * n, [None] * n
    for j in range(n):
        if units[j][0] == "copy":
            streams[j] = bytes(units[j][1])
    if total is None:
        for j in searched:
            streams[j], infos[j], r = encode(ans[j], version, None if budget is None else int(budget[j]), rate)
            raws[j] = (r, ans[j])
        return streams, infos, None, None, raws
    copies = sum(len(units[j][1]) for j in range(n) if units[j][0] == "copy")
    left = max(total - copies, 0)
    caps = None if cap is None else [int(cap[j]) for j in searched]
    if searched:
        sizes, rec, _ = FR.allot([curve(ans[j], version) for j in searched], left, caps)
    else:
        sizes, rec = [], dict(totalBytes=0, leastBytes=0, usedBytes=0, sqErr=0, nSteps=0, stepsTaken=0, fits=1)
    for j, b in zip(searched, FR.budgets(sizes, caps)):
        streams[j], infos[j], r = encode(ans[j], version, b, rate)
        raws[j] = (r, ans[j])
    rec = dict(rec, totalBytes=total, leastBytes=rec["leastBytes"] + copies, usedBytes=rec["usedBytes"] + copies,
               sqErr=sum(infos[j][6] for j in searched))
    rec["fits"] = int(rec["leastBytes"] <= total)
    allot = [len(s) for s in streams]
    for j, s in zip(searched, sizes):
        allot[j] = s
    return streams, infos, rec, allot, raws


# ------------------------------------------------------------------------------------------------------------ the sources

@functools.lru_cache(maxsize=None)
def filter_table():
    c, inc = D.resample_filter_default()
    return np.asarray(c, np.float32), int(inc)


def converted(values, rate, channels=1, level=None):
    """any-rate PCM as the encoder reads it: resampled, then levelled (level None: as it is)"""
    c, inc = filter_table()
    y = RS.resample(np.asarray(values, np.float32), rate, c, inc, channels)
    return y if level is None else level_ref.apply(y, level)[0]


def file_pcm(b):
    """a WAV or FLAC file's signal at 31 250 Hz"""
    st, mono, d = (flac_ref if b[:4] == b"fLaC" else wav_ref).decode(b)
    assert st == 0
    return converted(mono, d["rate"] if "rate" in d else d["sampleRate"])


def stream_units(checker, srcs, version, budget=None, total=None, cap=None, reencode_all=False):
    """existing streams (bytes, os) as units: copied by the rule, else decoded as the recipe plays them"""
    units = []
    for j, (s, os_) in enumerate(srcs):
        copyable = T.action(s, os_, version) == T.COPIED
        if copied(copyable, len(s), j, budget, total, cap, reencode_all):
            units.append(("copy", s))
        else:
            units.append(("pcm", E.to_float(T.decoded(checker, s, os_))))
    return units


def file_units(checker, files, version, budget=None, total=None, cap=None, reencode_all=False):
    units = []
    for j, b in enumerate(files):
        if b[:4] == b"DCSa":
            os_, s = D.dcsa_parse(b)
            units += stream_units(checker, [(s, os_)], version, None if budget is None else [budget[j]], total,
                                  None if cap is None else [cap[j]], reencode_all)
        else:
            units.append(("pcm", file_pcm(b)))
    return units


# ---------------------------------------------------------------------------------------------------------- the small lists

def _tone(n, seed, amp):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return amp * (0.6 * np.sin(2 * np.pi * t * (0.01 + 0.02 * rng.random())) + 0.4 * (rng.random(n) * 2 - 1))


def dcsa(fmt, frames, seed):
    s = make_stream(fmt, frames, seed=seed)
    return D.dcsa_header(D.format_os(fmt), len(s)) + s


@functools.lru_cache(maxsize=None)
def mixed_files(version):
    """the interleaved list: a stereo 44.1 kHz WAV, a container of another family (searched), a mono 22.05 kHz FLAC, a
    container of the target's family (copyable), a near-silent WAV"""
    other = D.FMT_93B_T1 if version == 0x9400 else D.FMT_94_T1_S0
    own = {0x9400: D.FMT_94_T0, 0x9302: D.FMT_93B_T1, 0x9301: D.FMT_93_T0}[version]
    stereo = np.round(_tone(2 * 1000, 0xA1, 0.5) * 32767).astype(np.int64)
    quiet = np.round(_tone(700, 0xA3, 0.0004) * 32767).astype(np.int64)
    flac, _ = flac_cases.simple(0xA2, 22050, 1, 16, [(384, 0, [flac_cases.S("fixed", order=2, k=10)]),
                                                     (200, 0, [flac_cases.S("verbatim")])])
    own_s = make_stream(own, 3, seed=0xA5)
    return (wav_cases.wav("s16", 2, 44100, stereo), dcsa(other, 2, 0xA4), flac,
            D.dcsa_header(OS_OF[version], len(own_s)) + own_s, wav_cases.wav("s16", 1, 44100, quiet))


def rate_budgets(units, rate):
    """the bytes the rate gives each searched unit (18 header bytes and the whole bytes of its bits); a copy's own length"""
    return [len(u[1]) if u[0] == "copy" else 18 + (rate * ((len(u[1]) + 239) // 240) * 240 // 31250) // 8 for u in units]


def digest(streams, infos, rec=None):
    h = hashlib.sha256()
    for s, i in zip(streams, infos):
        h.update(len(s).to_bytes(4, "little") + s + repr(tuple(int(v) for v in i)).encode())
    if rec is not None:
        h.update(repr(FR.record_tuple(rec)).encode())
    return h.hexdigest()


def info_of(rec):
    return tuple(int(rec[k]) for k in INFO_KEYS)
