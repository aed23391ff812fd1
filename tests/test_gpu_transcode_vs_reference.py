"""dcs_transcode_streams on seeded cases (tests/transcode_cases.py), path by path: the reference composition's bytes on every
case the screen keeps and the restatement's bytes and info on every case; the device-planned decode, the host-planned retry
after the device planner flags a list, and the host walk on either side of its boundary, each with a precondition that shows
the path was taken; the same bytes under every decode knob and whatever the batch around a source; no state carried from
one call to the next; errors named by the caller's index; the capacity protocol after a fallback."""
import ctypes
import re

import numpy as np
import pytest

import dcsexplorer_amd as D
import transcode_cases as X
import transcode_ref as T
from dcsexplorer_amd.api import ERR_BAD_STREAM, ERR_CAPACITY
from test_gpu_transcode import FMT
from util import corrupt, make_stream

pytestmark = pytest.mark.gpu

SEED = 0x7C0D               # the CPU module's cases (test_transcode_vs_reference.py)
N_SETS = 540
N_DROPPED = 9
SPECIAL = [("flagged", k) for k in range(3)] + [("walk", w) for w in ("2048", "2049", "eq", "gt")] + [("knobs",), ("easy",)] \
    + [("fills", ti, ra) for ti in range(len(X.TARGETS)) for ra in (0, 1)]


@pytest.fixture(scope="module")
def sets():
    return {k: X.set_of(k) for k in X.keys(SEED, N_SETS, N_DROPPED) + SPECIAL}


@pytest.fixture(scope="module")
def expected(sets):
    res = X.expect_all(list(sets), with_reference=X.reference_available())
    if X.reference_available():
        print("\nGPU transcoding cases vs reference, re-encoded sources by source layout x target:\n"
              + X.format_tally(X.tally({k: v for k, v in res.items() if k[0] in ("set", "dropped")})))
    return res


def call(ctx, s, sources=None):
    """one dcs_transcode_streams call on the set's target, params, flag, volume and level -> (list of bytes, info)"""
    srcs = s.sources if sources is None else sources
    version = s.target[0]
    kw = dict(s.params, volume=s.volume, level=s.level)
    if s.dcsa:
        boxes = [D.dcsa_header(src.os, len(src.data)) + src.data for src in srcs]
        out, info = ctx.transcode_dcsa(boxes, version, FMT[s.target], s.reencode_all, **kw)
        for box in out:
            assert box[:36] == D.dcsa_header(D.TRANSCODE_OS[version], len(box) - 36)
        return [D.dcsa_parse(b)[1] for b in out], info
    return ctx.transcode_streams([src.data for src in srcs], [src.os for src in srcs], version, FMT[s.target], s.reencode_all, **kw)


def refused(ctx, s, sources=None):
    """-> the caller's index the call's DCS_ERR_BAD_STREAM names"""
    with pytest.raises(D.DcsError) as e:
        call(ctx, s, sources)
    assert e.value.status == ERR_BAD_STREAM, str(e.value)
    m = re.search(r"stream (\d+):", str(e.value))
    assert m, str(e.value)
    return int(m.group(1))


def reencoded(s, sources=None):
    """the re-encoded sources as device_path takes them"""
    return [(src.os, src.data, s.volume, s.level) for src in (s.sources if sources is None else sources)
            if T.action(src.data, src.os, s.target[0], s.reencode_all) == T.REENCODED]


def path_of(ctx, s, sources=None):
    """which decode dcs_transcode_streams runs for the list: "copy" (nothing re-encoded), "host-walk" (the host-walk rule,
    restated), "device" (the device planner serves the re-encoded list) or "flagged" (it cannot: the host-planned retry)"""
    re_ = reencoded(s, sources)
    if not re_:
        return "copy"
    if X.walks_on_host([X.frames(d) for _, d, _, _ in re_]):
        return "host-walk"
    try:
        ctx.device_path(re_, extra_frames=1).close()
        return "device"
    except D.DcsError as e:
        assert e.status == ERR_BAD_STREAM and "cannot serve" in str(e), str(e)
        return "flagged"


def check_bytes(got, info, es, what):
    """bytes and info rows against the expectations; -> list of mismatches"""
    bad = []
    assert len(got) == len(es) == len(info)
    for g, inf, e in zip(got, info, es):
        want = e.ref if e.status == "kept" else e.want
        if g != e.want or (want is not None and g != want):
            bad.append("%s %s (%s): %d bytes, want %d" % (what, e.name, e.status, len(g), len(e.want)))
            continue
        assert inf["action"] == e.action and inf["srcFrames"] == X.frames(g) - (1 if e.action == T.REENCODED else 0), e.name
        assert inf["enc"]["nBytes"] == len(g) and inf["enc"]["nFrames"] == X.frames(g), e.name
        if e.action == T.COPIED:
            assert inf["enc"]["bandsToKeep"] == -1 and inf["enc"]["formatType"] == g[2] >> 7, e.name
        else:
            assert (inf["enc"]["formatType"], inf["enc"]["formatSubType"]) == tuple(e.win), e.name
            assert inf["enc"]["bandsToKeep"] == e.keep, e.name
    return bad


@pytest.fixture(scope="module")
def results(gpu_ctx, sets, expected):
    """every case set in one call of its own -> {key: (bytes, info) or the index a refused call names}"""
    out = {}
    for key, s in sets.items():
        if key[0] in ("set", "dropped"):
            fb = X.first_bad(s, expected[key])
            out[key] = refused(gpu_ctx, s) if fb is not None else call(gpu_ctx, s)
    return out


def test_every_set_in_one_call(sets, expected, results):
    bad, n_ref = [], 0
    for key, r in results.items():
        es = expected[key]
        fb = X.first_bad(sets[key], es)
        if fb is not None:
            assert r == fb, (key, r, fb)
            continue
        bad += check_bytes(r[0], r[1], es, "%r" % (key,))
        n_ref += sum(e.status == "kept" for e in es)
    assert not bad, "%d sources differ:\n%s" % (len(bad), "\n".join(bad[:20]))
    if X.reference_available():
        assert n_ref >= 1000
    # the OS93a all-bands-dropped stream: refused wherever it is re-encoded, copied verbatim for an OS93a target
    dropped = [k for k in results if k[0] == "dropped"]
    assert sum(isinstance(results[k], int) for k in dropped) == 8
    assert all(not isinstance(results[k], int) for k in dropped if sets[k].target[0] == 0x9301)


def test_every_path_is_taken(gpu_ctx, sets, expected):
    paths = {}
    for key, s in sets.items():
        if key[0] == "set":
            paths.setdefault(path_of(gpu_ctx, s), []).append(key)
    counts = {p: len(v) for p, v in paths.items()}
    assert counts.get("device", 0) >= 100 and counts.get("flagged", 0) >= 20, counts


@pytest.mark.parametrize("fpw", [4, 8, 16])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_flagged_list_is_decoded_again_on_the_host(gpu_ctx, sets, expected, fpw, k):
    s, es = sets["flagged", k], expected["flagged", k]
    try:
        gpu_ctx.set_frames_per_wave(fpw)
        assert path_of(gpu_ctx, s) == "flagged"
        got, info = call(gpu_ctx, s)
        assert not check_bytes(got, info, es, "flagged")
        for src, g in zip(s.sources, got):
            assert call(gpu_ctx, s, [src])[0][0] == g, src.name
    finally:
        gpu_ctx.set_frames_per_wave(0)


@pytest.mark.parametrize("which,path", [("2048", "device"), ("2049", "host-walk"), ("eq", "device"), ("gt", "host-walk")])
def test_host_walk_boundary(gpu_ctx, sets, expected, which, path):
    s, es = sets["walk", which], expected["walk", which]
    assert path_of(gpu_ctx, s) == path
    got, info = call(gpu_ctx, s)
    assert not check_bytes(got, info, es, "walk-" + which)
    done = set()
    for src, g in zip(s.sources, got):
        if src.data not in done:
            done.add(src.data)
            assert call(gpu_ctx, s, [src])[0][0] == g, src.name
    assert len(done) == (1 if which in ("2048", "2049") else 3)


KNOBS = [dict(fpw=f, handoff=h) for f in (4, 8, 16) for h in (True, False)] + [dict(fpc=1), dict(order_seed=0x5EED), dict(no_xcd=True)]


def test_knobs_do_not_change_the_bytes(gpu_ctx, sets, expected):
    s, es = sets["knobs",], expected["knobs",]
    assert path_of(gpu_ctx, s) == "flagged"
    try:
        for knob in KNOBS:
            gpu_ctx.set_frames_per_wave(knob.get("fpw", 0))
            gpu_ctx.set_tail_handoff(knob.get("handoff", True))
            gpu_ctx.set_frames_per_chunk(knob.get("fpc", 0))
            gpu_ctx.set_test_hooks(chunk_order_seed=knob.get("order_seed", 0), no_xcd_ranges=knob.get("no_xcd", False))
            got, info = call(gpu_ctx, s)
            assert not check_bytes(got, info, es, "knobs %r" % knob), knob
    finally:
        gpu_ctx.set_frames_per_wave(0)
        gpu_ctx.set_tail_handoff(True)
        gpu_ctx.set_frames_per_chunk(0)
        gpu_ctx.set_test_hooks(0)


def _reencoded_frames(s, sources):
    return sum(X.frames(src.data) + 1 for src in sources if T.action(src.data, src.os, s.target[0], s.reencode_all) == T.REENCODED)


def test_batch_composition(gpu_ctx, sets, expected, results):
    """each set shuffled; the sets of one target at the recipe and defaults merged into one shuffled call; those sources
    interleaved with 1-frame sources and copies so that the re-encoded frames are a multiple of neither 4 nor 64; one call of
    over 2 000 sources"""
    rng = np.random.default_rng(SEED)
    by_name = {}
    groups = {}
    for key, r in results.items():
        s = sets[key]
        if isinstance(r, int):
            continue
        for src, g in zip(s.sources, r[0]):
            by_name[src.name] = g
        order = list(rng.permutation(len(s.sources)))
        got, _ = call(gpu_ctx, s, [s.sources[i] for i in order])
        for i, g in zip(order, got):
            assert g == r[0][i], ("shuffled", s.sources[i].name)
        if key[0] == "set" and not s.dcsa and s.params == sets["easy",].params and (s.volume, s.level) == X.RECIPE:
            groups.setdefault((s.target, s.reencode_all), []).append(s)
    assert len(groups) >= 12
    n_big = 0
    for (target, ra), members in sorted(groups.items()):
        s = members[0]
        srcs = [src for m in members for src in m.sources]
        order = list(rng.permutation(len(srcs)))
        got, _ = call(gpu_ctx, s, [srcs[i] for i in order])
        for i, g in zip(order, got):
            assert g == by_name[srcs[i].name], ("merged", srcs[i].name)
        fills = sets["fills", X.TARGETS.index(target), int(ra)]
        for e, f in zip(expected[fills.key], fills.sources):
            by_name[f.name] = e.want
        n_fill = 2100 if n_big == 0 else len(srcs)
        mixed, j = [], 0
        for src in srcs:
            mixed.append(src)
            for _ in range(-(-n_fill // len(srcs))):
                mixed.append(fills.sources[j % len(fills.sources)])
                j += 1
        while _reencoded_frames(s, mixed) % 4 == 0 or _reencoded_frames(s, mixed) % 64 == 0:
            mixed.append(fills.sources[j % len(fills.sources)])
            j += 1
        if n_big == 0:
            assert len(mixed) > 2000
        n_big += 1
        got, _ = call(gpu_ctx, s, mixed)
        for src, g in zip(mixed, got):
            assert g == by_name[src.name], ("interleaved", src.name)


def test_context_state_is_not_carried_over(gpu_ctx, sets, expected):
    """a flagged list, an easy list, a list refused with BAD_STREAM, the easy list again: every result its own"""
    flagged, easy = sets["knobs",], sets["easy",]
    assert path_of(gpu_ctx, flagged) == "flagged" and path_of(gpu_ctx, easy) == "device"
    failing = X.set_of(("dropped", SEED, 0))
    assert X.first_bad(failing, expected[failing.key]) is not None
    for s in (flagged, easy):
        got, info = call(gpu_ctx, s)
        assert not check_bytes(got, info, expected[s.key], "state")
    assert refused(gpu_ctx, failing) == X.first_bad(failing, expected[failing.key])
    got, info = call(gpu_ctx, easy)
    assert not check_bytes(got, info, expected[easy.key], "state, again")


def _corrupted():
    """an OS93b stream whose index walk stops early (re-encoded into a 1994+ target, where it must be refused)"""
    base = make_stream(D.FMT_93B_T1, 40, seed=0xBAD)
    for seed in range(1, 200):
        s = corrupt(base, seed, nflips=6)
        _, inf = D.index_stream(D.OS93B, s)
        if inf.nValidFrames < inf.nFrames:
            return s
    raise AssertionError("no corruption seed stops the stream")


def _dropped_source(sets):
    return next(src for src in sets["dropped", SEED, 0].sources if src.bad)


def test_bad_source_is_named_by_the_callers_index(gpu_ctx, sets):
    """behind copies, so that the caller's index is not the re-encode index: on the device-planned path and after a fallback"""
    bad = _dropped_source(sets)
    easy, flagged = sets["easy",], sets["flagged", 0]
    again = lambda src: T.action(src.data, src.os, easy.target[0]) == T.REENCODED
    copies = [src for src in flagged.sources if "/copy-" in src.name]
    sat = [src for src in flagged.sources if "-p4-" in src.name and again(src)]
    easy_re = [src for src in easy.sources if again(src)]
    assert flagged.target == easy.target and len(copies) >= 2 and len(sat) >= 2 and len(easy_re) >= 2
    # the device planner refuses a list with the all-dropped OS93a stream in it; a corrupted stream whose index walk stops
    # early is planned on the device
    corrupted = X.Source("corrupted", _corrupted(), D.OS93B, True)
    assert again(corrupted)
    on_device = [copies[0], copies[1], easy_re[0], copies[0], corrupted, easy_re[1]]
    for bad_src in (corrupted, bad):
        after_fallback = [copies[0], sat[0], copies[1], copies[0], bad_src, sat[1]]
        for sources, path in ((on_device, "device"), (after_fallback, "flagged")):
            s = easy._replace(sources=sources)
            assert path_of(gpu_ctx, s, sources) == path, [src.name for src in sources]
            assert refused(gpu_ctx, s, sources) == 4, path
    # and the context still works
    got, info = call(gpu_ctx, easy)
    assert got[0] == call(gpu_ctx, easy, easy.sources[:1])[0][0]


def test_capacity_after_a_fallback(gpu_ctx, sets, expected):
    s, es = sets["flagged", 0], expected["flagged", 0]
    assert path_of(gpu_ctx, s) == "flagged"
    want = [e.want for e in es]
    L = D.load_library()
    p = D.transcode_params(s.target[0], FMT[s.target], **s.params)
    refs, keep = D.api._transcode_refs([src.data for src in s.sources], [src.os for src in s.sources], s.volume, s.level, 0xFF)
    total = sum(len(x) for x in want)
    out = np.full(total + 64, 0xA5, np.uint8)
    offs = np.zeros(len(want) + 1, np.uint64)
    st = L.dcs_transcode_streams(gpu_ctx.h, refs, len(want), ctypes.byref(p), 0, D.api._ptr(out), total - 1, D.api._ptr(offs), None)
    assert st == ERR_CAPACITY
    assert list(np.diff(offs)) == [len(x) for x in want]
    assert (out == 0xA5).all(), "a refused call wrote to the output buffer"
    offs[:] = 0
    st = L.dcs_transcode_streams(gpu_ctx.h, refs, len(want), ctypes.byref(p), 0, D.api._ptr(out), total, D.api._ptr(offs), None)
    assert st == 0 and out[:total].tobytes() == b"".join(want) and (out[total:] == 0xA5).all()
    assert list(np.diff(offs)) == [len(x) for x in want]
