"""Seeded transcoding cases, and their expected bytes (test infrastructure).

A case set is one dcs_transcode_streams call: a list of sources, each with the OS it plays under, and one target, one draw
of CompressionParams, the REENCODE_ALL flag, and the volume and level the recipe plays the sources at.  Everything is a pure
function of its key, so a spawned worker rebuilds a set from the key instead of receiving the bytes (as tests/enc_cases.py
does for the encoders).

The sources aim at the paths of dcs_transcode_streams: synthetic streams of every layout and profile at frame counts around
the 4/8/16-frame wavefronts and the chunk sizes; sources the device planner refuses (saturated frames, large frames,
truncated streams), which send the list to the host-planned retry; streams the library's own encoders write (int16 edges,
Nyquist squares, frame-edge impulses, silence, every band at 0 bits, the masked shift); the encoder recordings; trailing
bytes past the stream; DCSa containers.  The recipe plays them at 0x67 / 0xFF mostly, and also loud enough to clip
(0xFF / 0xFF), at volume 0 (all-zero PCM), volume 1, and at a low level.

expect() gives every source of a set what the library must write: the source's own bytes where the rule copies it, else the
restatement's (tests/transcode_ref.py: the oracle's decode, the numpy encoders), screened against the compiled reference
composition (its decoder, then oracle/_ref/dcs_encref) as enc_cases.check() screens an encoder case.  A source whose decode
reports an error word (the OS93a stream with every band dropped, whose all-0xFF header decodes FATAL) is BAD: a call that
re-encodes it fails with DCS_ERR_BAD_STREAM and names it."""
import collections
import concurrent.futures
import functools
import multiprocessing
import os

import numpy as np

import dcsexplorer_amd as D
import enc_cases as C
import enc_ref as E
import transcode_ref as T
from util import make_stream

HERE = os.path.dirname(os.path.abspath(__file__))

# every target the encoders offer: (version, type, sub-type), -1 = wildcard (as test_transcode_host.TARGETS)
TARGETS = [(0x9400, -1, -1), (0x9400, 0, 0), (0x9400, 0, 3), (0x9400, 1, 0), (0x9400, 1, 3),
           (0x9302, -1, -1), (0x9302, 0, -1), (0x9302, 1, -1), (0x9301, 0, -1)]
FAMILY = {0x9400: "94", 0x9302: "93b", 0x9301: "93a"}
# the source layouts of the tally: the six unpack layouts, read from the OS and the header's type and sub-type bits
LAYOUTS = ["93-T0", "93b-T1", "93a-T1", "94-T0", "94-T1s0", "94-T1s3"]
# frame counts around the 4/8/16-frame wavefronts and the chunk sizes, the host-walk threshold (2 048) among them
FRAMES = [1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 2047, 2048, 2049]
FRAME_WEIGHTS = np.array([4, 3, 3, 3, 3, 3, 3, 3, 3, 1.5, 1.5, 1.5, 0.6, 0.2, 0.2, 0.2])
RECIPE = (0x67, 0xFF)
KINDS = ["synth", "flagged", "encoded", "recordings", "mixed", "synth", "encoded", "mixed"]

Source = collections.namedtuple("Source", "name data os bad")
Set = collections.namedtuple("Set", "key sources target params reencode_all volume level dcsa")
Expected = collections.namedtuple("Expected", "name layout target action status want ref win keep fired pcm_same")


def layout_of(data, os_):
    if os_ in (D.OS93A, D.OS93B):
        return "93-T0" if not data[2] & 0x80 else ("93a-T1" if os_ == D.OS93A else "93b-T1")
    if not data[2] & 0x80:
        return "94-T0"
    return "94-T1s0" if len(data) < 5 or not data[4] & 0x80 else "94-T1s3"


def frames(data):
    return (data[0] << 8) | data[1]


def decode_stops(data, os_):
    """the oracle's per-frame error flags (ORC_ERR_STOP, ORC_ERR_FATAL) over the stream's frames: nonzero = the library's
    decode reports an error word, and a transcode that re-encodes the source fails with DCS_ERR_BAD_STREAM"""
    return int(np.bitwise_or.reduce(_oracle().decompress(os_, data, 0x4000, frames(data))[3]))


def _nframes(rng, short=False):
    w = FRAME_WEIGHTS[:9] if short else FRAME_WEIGHTS
    return int(FRAMES[rng.choice(len(w), p=w / w.sum())])


def _synth(rng, name, nframes=None, profile=None, dcsa=False):
    fmt = int(rng.integers(6))
    profile = int(rng.choice([0, 0, 1, 2, 3, 5])) if profile is None else profile
    stride = 16 if rng.random() < 0.6 else int(rng.choice([4, 7, 8, 12]))
    s = make_stream(fmt, nframes or _nframes(rng), seed=int(rng.integers(1 << 30)), profile=profile, stride_from=stride)
    os_ = D.format_os(fmt, prefer_95=bool(rng.random() < 0.5) and not dcsa, prefer_93a=bool(rng.random() < 0.5))
    return Source("%s/synth-f%d-p%d-s%d" % (name, fmt, profile, stride), s, os_, False)


def _truncated(rng, name):
    """a stream cut short by a few bytes that still indexes and decodes every frame without an error word (bytes past the end
    read as zero; cut further, the zeros decode to a band type the reference leaves undefined, and the decoder says FATAL)"""
    for _ in range(64):
        fmt = int(rng.integers(6))
        full = make_stream(fmt, int(rng.integers(8, 70)), seed=int(rng.integers(1 << 30)))
        os_ = D.format_os(fmt)
        last = None
        for cut in range(1, 17):
            _, inf = D.index_stream(os_, full[:-cut])
            if inf.nValidFrames != inf.nFrames or decode_stops(full[:-cut], os_):
                break
            last = full[:-cut]
        if last is not None:
            return Source("%s/truncated-f%d-%d" % (name, fmt, len(full) - len(last)), last, os_, False)
    raise AssertionError("no truncation keeps every frame")


def _flagged(rng, name):
    """a source the device planner refuses: saturated frames, large frames, or a truncated stream"""
    u = rng.random()
    if u < 0.45:
        return _synth(rng, name, int(rng.integers(8, 80)), profile=4)
    if u < 0.75:
        fmt = int(rng.choice([0, 1, 3]))
        s = make_stream(fmt, int(rng.integers(8, 80)), seed=int(rng.integers(1 << 30)), profile=4, nbands=10)
        return Source("%s/large-f%d" % (name, fmt), s, D.format_os(fmt, prefer_95=bool(fmt & 1), prefer_93a=bool(fmt & 1)), False)
    return _truncated(rng, name)


_SIGNALS = [("int16", C._int16_edge), ("square", C._square), ("impulse", C._impulse), ("silence", lambda rng, n: np.zeros(n, C.F32)),
            ("music", C._music), ("unit", C._unit)]


def _encoded(rng, name, dropped=False):
    """a stream the library's encoders write: a restatement's output on an enc_cases signal"""
    fam = "93a" if dropped else str(rng.choice(list(C.FAMILIES)))
    version, lays = C.FAMILIES[fam]
    lay = "T0" if dropped else str(rng.choice(list(lays)))
    typ, sub = lays[lay]
    kind, fn = _SIGNALS[4] if dropped else _SIGNALS[rng.integers(len(_SIGNALS))]
    n = int(rng.integers(1, 48)) * 240 - int(rng.integers(0, 240))
    x = fn(rng, max(n, 1))
    p = C._params(rng) if rng.random() < 0.6 else dict(E.DEFAULTS)
    if rng.random() < 0.4:
        p["targetBitRate"] = int(rng.choice([1, 2000000, 100000000]))
    if dropped:
        p["powerBandCutoff"] = 0.0                      # every band dropped: an all-0xFF header
    s, win, _, _ = C.restate(C.Case(name, x, fam, lay, version, typ, sub, p))
    all_dropped = fam == "93a" and s[2:18] == b"\xff" * 16
    if all_dropped != dropped:
        return _encoded(rng, name, dropped)
    os_ = D.OS93A if fam == "93a" else D.OS93B if fam == "93b" else (D.OS95 if win[1] == 3 else D.OS94)
    return Source("%s/enc-%s-%s-%s-%d" % (name, fam, lay, kind, len(x)), s, os_, dropped)


@functools.lru_cache(maxsize=1)
def _recordings():
    rec = np.load(os.path.join(HERE, "golden", "encoder_golden.npz"))
    os_of = {"94": D.OS94, "93b": D.OS93B, "93a": D.OS93A}
    return [(k, rec[k].tobytes(), os_of[k.split("-")[1]]) for k in sorted(k for k in rec.keys() if k.endswith("/stream"))]


def _recording(rng, name):
    k, s, os_ = _recordings()[rng.integers(24)]
    return Source("%s/rec-%s" % (name, k.split("/")[0]), s, os_, False)


def _volume_level(rng):
    u = rng.random()
    if u < 0.6:
        return RECIPE
    return [(0xFF, 0xFF), (0, 0xFF), (1, 0xFF), (0x67, int(rng.choice([1, 0x10, 0x40])))][rng.integers(4)]


def case_set(seed, k):
    """the k-th set of generator `seed`: target TARGETS[k % 9], sources of kind KINDS[(k // 9) % 8]"""
    rng = np.random.default_rng([seed, k])
    name = "s%x-%d" % (seed, k)
    target = TARGETS[k % len(TARGETS)]
    kind = KINDS[(k // len(TARGETS)) % len(KINDS)]
    dcsa = rng.random() < 0.12
    draw = {"synth": lambda: _synth(rng, name, dcsa=dcsa),
            "flagged": lambda: _flagged(rng, name) if rng.random() < 0.5 else _synth(rng, name, _nframes(rng, True), 0, dcsa),
            "encoded": lambda: _encoded(rng, name),
            "recordings": lambda: _recording(rng, name)}
    draw["mixed"] = lambda: draw[["synth", "flagged", "encoded", "recordings"][rng.integers(4)]]()
    sources = []
    for j in range(int(rng.integers(3, 9))):
        s = draw[kind]()
        if dcsa and s.os == D.OS95:
            s = s._replace(os=D.OS94)                    # the container does not tell OS95 from OS94
        if rng.random() < 0.12 and not s.name.split("/")[1].startswith("truncated"):
            s = s._replace(name=s.name + "+tail", data=s.data + rng.integers(0, 256, int(rng.integers(1, 10)), dtype=np.uint8).tobytes())
        sources.append(s._replace(name="%s/%d" % (s.name, j)))
    params = C._params(rng) if rng.random() < 0.5 else dict(E.DEFAULTS)
    volume, level = _volume_level(rng)
    return Set(("set", seed, k), sources, target, params, bool(rng.random() < 0.8), volume, level, dcsa)


def dropped_set(seed, k):
    """the OS93a all-bands-dropped stream behind copies and good sources: BAD_STREAM where re-encoded, copied for 0x9301"""
    rng = np.random.default_rng([seed, k, 0xD0])
    name = "d%x-%d" % (seed, k)
    target = TARGETS[k % len(TARGETS)]
    sources = [_synth(rng, name, _nframes(rng, True), 0) for _ in range(int(rng.integers(1, 4)))]
    sources.append(_encoded(rng, name, dropped=True))
    sources += [_synth(rng, name, _nframes(rng, True), 0) for _ in range(int(rng.integers(0, 3)))]
    sources = [s._replace(name="%s/%d" % (s.name, j)) for j, s in enumerate(sources)]
    return Set(("dropped", seed, k), sources, target, dict(E.DEFAULTS), False, 0x67, 0xFF, False)


def keys(seed, n_sets, n_dropped=0):
    return [("set", seed, k) for k in range(n_sets)] + [("dropped", seed, k) for k in range(n_dropped)]


# ------------------------------------------------------------------------------------ lists built for one path each
def _numbered(sources):
    return [s._replace(name="%s/%d" % (s.name, j)) for j, s in enumerate(sources)]


def _copy_for(rng, name, target):
    """a source the rule copies into `target` (without REENCODE_ALL)"""
    fmt = {0x9400: int(rng.choice([D.FMT_94_T0, D.FMT_94_T1_S0, D.FMT_94_T1_S3])), 0x9302: D.FMT_93B_T1, 0x9301: D.FMT_93_T0}[target[0]]
    os_ = D.OS94 if target[0] == 0x9400 else D.OS93B if target[0] == 0x9302 else D.OS93A
    return Source("%s/copy-f%d" % (name, fmt), make_stream(fmt, int(rng.integers(5, 60)), seed=int(rng.integers(1 << 30))), os_, False)


def flagged_list(k):
    """saturated, large and truncated sources among easy ones and copies: the device planner refuses the re-encoded list"""
    rng = np.random.default_rng([0xF1A6, k])
    name = "flagged%d" % k
    target = [(0x9400, -1, -1), (0x9302, -1, -1), (0x9301, 0, -1)][k % 3]
    sat = lambda: _synth(rng, name, int(rng.integers(20, 70)), profile=4)
    easy = lambda: _synth(rng, name, _nframes(rng, True), 0)
    copy = lambda: _copy_for(rng, name, target)
    large = lambda: _flagged(np.random.default_rng([0xF1A6, k, 1]), name)
    sources = [sat(), easy(), copy(), sat(), large(), easy(), copy(), _truncated(rng, name), sat(), easy()]
    return Set(("flagged", k), _numbered(sources), target, dict(E.DEFAULTS), False, 0x67, 0xFF, False)


# the host-walk rule of dcs_transcode_streams: a re-encoded source longer than this that has less than 1/64 of the re-encoded
# list's frames beside it sends the list to the host walk and the host-planned batch
HOST_WALK_FRAMES = 2048


def walks_on_host(counts):
    longest, total = max(counts), sum(counts)
    return longest > HOST_WALK_FRAMES and longest * 64 > total


def walk_list(which):
    """"2048" / "2049": one source of that many frames alone; "eq": a 2 049-frame source with 1 000-frame fillers and a
    remainder, longest * 64 == total (walked on the device); "gt": one frame fewer, longest * 64 > total (on the host)"""
    rng = np.random.default_rng([0x3A1C, 0])
    mk = lambda n, tag: Source("walk-%s/%s-%d" % (which, tag, n), make_stream(D.FMT_93B_T1, n, seed=int(rng.integers(1 << 30))), D.OS93B, False)
    long_, filler = mk(2049, "long"), mk(1000, "filler")
    if which in ("2048", "2049"):
        sources = [mk(int(which), "alone")]
    else:
        rem = 2049 * 64 - 2049 - 129 * 1000 - (0 if which == "eq" else 1)
        sources = [filler] * 64 + [long_] + [filler] * 65 + [mk(rem, "rem")]
    return Set(("walk", which), _numbered(sources), (0x9400, -1, -1), dict(E.DEFAULTS), False, 0x67, 0xFF, False)


def knobs_list():
    """a flagged sub-list, copies, and ragged lengths from 1 frame to 1 000 (several decode chunks)"""
    rng = np.random.default_rng([0x4B0B, 0])
    name, target = "knobs", (0x9400, -1, -1)
    sources = [_synth(rng, name, n, 0) for n in (1, 17, 64, 257, 1000, 2, 63, 65)]
    sources[1:1] = [_synth(rng, name, 40, profile=4), _copy_for(rng, name, target)]
    sources[6:6] = [_flagged(rng, name), _copy_for(rng, name, target), _synth(rng, name, 33, profile=4)]
    sources.append(_encoded(rng, name))
    return Set(("knobs",), _numbered(sources), target, dict(E.DEFAULTS), False, 0x67, 0xFF, False)


def easy_list():
    """profile-0 sources of every layout, and copies: served by the device planner"""
    rng = np.random.default_rng([0xEA5E, 0])
    target = (0x9400, -1, -1)
    sources = [Source("easy/synth-f%d" % fmt, make_stream(fmt, 17 + 6 * fmt, seed=int(rng.integers(1 << 30))), D.format_os(fmt), False)
               for fmt in range(6)]
    sources.insert(2, _copy_for(rng, "easy", target))
    return Set(("easy",), _numbered(sources), target, dict(E.DEFAULTS), False, 0x67, 0xFF, False)


def fill_list(ti, reencode_all):
    """1-frame sources of every layout (copies among them where the rule copies), for TARGETS[ti] at the recipe and defaults"""
    rng = np.random.default_rng([0xF111, ti, int(reencode_all)])
    sources = [Source("fill%d%d/f%d" % (ti, reencode_all, fmt), make_stream(fmt, 1, seed=int(rng.integers(1 << 30))),
                      D.format_os(fmt), False) for fmt in range(6)]
    return Set(("fills", ti, reencode_all), _numbered(sources), TARGETS[ti], dict(E.DEFAULTS), bool(reencode_all), 0x67, 0xFF, False)


def set_of(key):
    build = {"set": case_set, "dropped": dropped_set, "flagged": flagged_list, "walk": walk_list, "knobs": knobs_list,
             "easy": easy_list, "fills": fill_list}[key[0]]
    s = build(*key[1:])
    assert s.key == tuple(key), (s.key, key)
    return s


# ---------------------------------------------------------------------------------------------------------- expectation
@functools.lru_cache(maxsize=1)
def _oracle():
    from oracle.dcs_oracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=1)
def _reference():
    from oracle.dcs_oracle import Reference
    return Reference()


def reference_available():
    from oracle.dcs_oracle import reference_available as decoder_built
    return decoder_built() and C.reference_available()


def _defined(src):
    """the bytes the reference decoder is given: a truncated source with the zeros the library reads past its end (the
    reference reads whatever memory follows)"""
    return src.data + bytes(64) if "/truncated-" in src.name else src.data


def expect(s, with_reference=True):
    """-> [Expected] for every source of set s.  status: "copied", "bad" (re-encoded, decodes with an error word), or the
    enc_cases screen's "kept", "rule", "dropped", "unchecked"; want = the library's bytes (None for bad), ref = the compiled
    reference composition's where kept; pcm_same = the oracle's recipe PCM is the reference decoder's (None: not compared).
    Sources repeated in the list are worked out once."""
    version, typ, sub = s.target
    out, seen = [], {}
    for src in s.sources:
        act = T.action(src.data, src.os, version, s.reencode_all)
        lay = layout_of(src.data, src.os)
        memo = (src.data, src.os)
        if act == T.COPIED:
            e = Expected(src.name, lay, s.target, act, "copied", bytes(src.data), None, None, -1, 0, None)
        elif src.bad:
            assert decode_stops(src.data, src.os), src.name
            e = Expected(src.name, lay, s.target, act, "bad", None, None, None, None, 0, None)
        elif memo in seen:
            e = seen[memo]._replace(name=src.name)
        else:
            assert not decode_stops(src.data, src.os), src.name
            pcm = T.decoded(_oracle(), src.data, src.os, s.volume, s.level)
            same = np.array_equal(pcm, T.decoded(_reference(), _defined(src), src.os, s.volume, s.level)) if with_reference else None
            r = C.check(C.Case(src.name, E.to_float(pcm), FAMILY[version], "t%d%d" % (typ, sub), version, typ, sub, s.params),
                        with_reference)
            e = Expected(src.name, lay, s.target, act, r.status, r.want, r.ref, r.win, r.keep, r.fired, same)
            seen[memo] = e
        out.append(e)
    return out


def first_bad(s, expected):
    """the caller's index of the first source a call must refuse (re-encoded, bad), or None"""
    return next((i for i, e in enumerate(expected) if e.status == "bad"), None)


def _expect_key(key, with_reference):
    return key, expect(set_of(key), with_reference)


def expect_all(work, with_reference=True, workers=None):
    """expect() every set of the work items (keys, or callables that build a Set from nothing) in spawned workers
    -> {key: [Expected]}"""
    workers = workers or max(1, min(16, os.cpu_count() or 1))
    ctx = multiprocessing.get_context("spawn")
    with concurrent.futures.ProcessPoolExecutor(workers, mp_context=ctx) as pool:
        return dict(pool.map(_expect_key, work, [with_reference] * len(work)))


def tally(expected):
    """{(source layout, target): Counter of statuses}; re-encoded sources only"""
    out = {(lay, t): collections.Counter() for lay in LAYOUTS for t in TARGETS}
    for es in expected.values():
        for e in es:
            if e.status != "copied":
                out[e.layout, e.target][e.status] += 1
    return out


def format_tally(t):
    lines = ["%-8s %-18s %5s %5s %5s %5s" % ("source", "target", "kept", "rule", "drop", "bad")]
    for (lay, tg), c in t.items():
        lines.append("%-8s %-18s %5d %5d %5d %5d" % (lay, "%x/%d/%d" % tg, c["kept"], c["rule"], c["dropped"], c["bad"]))
    return "\n".join(lines)
