"""Both GPU encoders (dcs_encode_streams, dcs_encode93_streams) on seeded adversarial cases (tests/enc_cases.py): the
reference encoder's bytes on every case its UBSan build keeps (oracle/_ref/dcs_encref, where `build()` made it), the
restatement's bytes and info on every case, the same bytes whatever the batch around a stream, an output buffer used
exactly as far as the sizes say, and streams the GPU decoder turns into the oracle's PCM."""
import ctypes

import numpy as np
import pytest

import dcsexplorer_amd as D
import enc_cases as C
from dcsexplorer_amd.api import ERR_CAPACITY, _encode_input, _ptr

pytestmark = pytest.mark.gpu

SEED = 0x6E4C
N_SETS = 60                 # x 10 cases, 4 one-sample fillers each, + one 65 535-frame stream per family
FMT94 = {(-1, -1): None, (0, 0): D.FMT_94_T0, (0, 3): D.FMT_94_T0_S3, (1, 0): D.FMT_94_T1_S0, (1, 3): D.FMT_94_T1_S3}
FMT93 = {-1: None, 0: D.FMT_93_T0, 1: D.FMT_93B_T1}
OS93 = {0x9301: D.OS93A, 0x9302: D.OS93B}


def _sets():
    return {key: C.cases_of(key) for key in C.keys(SEED, N_SETS, with_fillers=True)}


def encode(ctx, cases):
    """one encoder call over cases that share family, layout and params -> (streams, info)"""
    c = cases[0]
    pcm = [x.pcm for x in cases]
    if c.family == "94":
        return ctx.encode_streams(pcm, FMT94[c.type, c.subtype], **c.params)
    return ctx.encode93_streams(pcm, OS93[c.version], FMT93[c.type], **c.params)


@pytest.fixture(scope="module")
def sets():
    return _sets()


@pytest.fixture(scope="module")
def expected(sets):
    res = C.check_all(list(sets), with_reference=C.reference_available())
    if C.reference_available():
        print("\nGPU cases vs reference, per layout:\n" + C.format_tally(C.tally(res)))
    return res


@pytest.fixture(scope="module")
def encoded(gpu_ctx, sets):
    """every set in one call of its own, in generated order -> {case name: (bytes, info row)}"""
    out = {}
    for key, cases in sets.items():
        streams, info = encode(gpu_ctx, cases)
        assert len(streams) == len(cases)
        for c, s, inf in zip(cases, streams, info):
            out[c.name] = (s, inf)
    return out


def _first_difference(a, b):
    i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return "%d vs %d bytes, first difference at byte %d" % (len(a), len(b), i)


def test_gpu_bytes_equal_the_reference(expected, encoded):
    if not C.reference_available():
        pytest.skip(C.MISSING)
    bad = []
    for name, r in expected.items():
        got = encoded[name][0]
        want = r.ref if r.status == "kept" else r.want        # dropped and rule cases: the library's bytes
        if got != want:
            bad.append("%s (%s): %s" % (name, r.status, _first_difference(got, want)))
    assert not bad, "%d GPU streams differ:\n%s" % (len(bad), "\n".join(bad[:20]))


def test_gpu_bytes_and_info_equal_the_restatement(sets, expected, encoded):
    bad = []
    for cases in sets.values():
        for c in cases:
            r = expected[c.name]
            got, inf = encoded[c.name]
            if got != r.want:
                bad.append("%s: %s" % (c.name, _first_difference(got, r.want)))
                continue
            assert (inf["formatType"], inf["formatSubType"]) == r.win, c.name
            assert inf["nFrames"] == (len(c.pcm) + 239) // 240 == (got[0] << 8 | got[1]), c.name
            assert inf["nBytes"] == len(got) and inf["bandsToKeep"] == r.keep, c.name
    assert not bad, "%d GPU streams differ from the restatement:\n%s" % (len(bad), "\n".join(bad[:20]))


def test_the_screen_is_not_hollow(expected):
    if not C.reference_available():
        pytest.skip(C.MISSING)
    t = C.tally(expected)
    assert sum(c["kept"] for c in t.values()) >= 0.9 * len(expected), C.format_tally(t)
    for fl, c in t.items():
        assert c["kept"] >= 20, (fl, C.format_tally(t))


def _interleave(cases, fills, n_fill):
    """the cases with n_fill 1-sample streams spread between them, and enough more that the call's frame count is a
    multiple of neither 4 nor 64 (the block sizes of the analysis, pack and walk kernels)"""
    frames = sum((len(c.pcm) + 239) // 240 for c in cases)
    while (frames + n_fill) % 4 == 0 or (frames + n_fill) % 64 == 0:
        n_fill += 1
    out, per = [], -(-n_fill // len(cases))
    for c in cases:
        out.append(c)
        for _ in range(min(per, n_fill)):
            out.append(fills[n_fill % len(fills)])
            n_fill -= 1
    assert n_fill == 0 and (frames + len(out) - len(cases)) % 4 != 0
    return out


def test_batch_composition(gpu_ctx, sets, expected, encoded):
    """every set shuffled in one call, a sample of its cases one call each, and interleaved with 1-sample streams; the
    first set of each family once more with over 2 000 streams in the call"""
    rng = np.random.default_rng(SEED)
    big = {}
    for key, cases in sets.items():
        if key[0] != "set":
            continue
        order = rng.permutation(len(cases))
        shuffled, _ = encode(gpu_ctx, [cases[i] for i in order])
        for i, s in zip(order, shuffled):
            assert s == encoded[cases[i].name][0], ("shuffled", cases[i].name)
        for i in rng.choice(len(cases), 2, replace=False):
            alone, _ = encode(gpu_ctx, [cases[i]])
            assert alone[0] == encoded[cases[i].name][0], ("alone", cases[i].name)
        fills = sets["fill", key[1], key[2]]
        n_fill = 2100 if big.setdefault(cases[0].family, key) == key else len(cases)
        mixed = _interleave(cases, fills, n_fill)
        streams, _ = encode(gpu_ctx, mixed)
        if n_fill > len(cases):
            assert len(mixed) > 2000
        for c, s in zip(mixed, streams):
            assert s == encoded[c.name][0] == expected[c.name].want, ("interleaved", c.name)
    assert len(big) == 3


def _raw(ctx, cases, cap, out, out_offs, info):
    c = cases[0]
    x, offs = _encode_input([k.pcm for k in cases])
    if c.family == "94":
        p = D.encode_params(FMT94[c.type, c.subtype], **c.params)
        fn = ctx.L.dcs_encode_streams
    else:
        p = D.encode93_params(OS93[c.version], FMT93[c.type], **c.params)
        fn = ctx.L.dcs_encode93_streams
    return fn(ctx.h, _ptr(x), _ptr(offs), len(cases), ctypes.byref(p), _ptr(out), cap, _ptr(out_offs), _ptr(info))


def test_output_buffer(gpu_ctx, sets, encoded):
    """every stream within its bound; an exactly sized buffer suffices and one byte less is refused with the size needed
    reported; nothing past the streams, or anything at all when refused, is written"""
    for cases in sets.values():
        for c in cases:
            bound = D.encode_bound(len(c.pcm)) if c.family == "94" else D.encode93_bound(len(c.pcm))
            assert 18 <= len(encoded[c.name][0]) <= bound, c.name
    seen = set()
    for key, cases in sets.items():
        if key[0] != "set" or (cases[0].family, cases[0].layout) in seen:
            continue
        seen.add((cases[0].family, cases[0].layout))
        want = [encoded[c.name][0] for c in cases]
        total = sum(len(s) for s in want)
        n = len(cases)
        out = np.full(total + 64, 0xA5, np.uint8)
        out_offs, info = np.zeros(n + 1, np.uint64), np.zeros(n, D.ENCODE_INFO_DTYPE)
        assert _raw(gpu_ctx, cases, total, out, out_offs, info) == 0
        assert out_offs.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in want])]).tolist()
        assert out[:total].tobytes() == b"".join(want)
        assert (out[total:] == 0xA5).all(), "bytes written past outOffsets[n]"
        out[:] = 0xA5
        out_offs[:] = 0
        assert _raw(gpu_ctx, cases, total - 1, out, out_offs, info) == ERR_CAPACITY
        assert int(out_offs[n]) == total
        assert (out == 0xA5).all(), "a refused call wrote to the output buffer"
    assert len(seen) == len(C.LAYOUTS)


def _decode_os(c, inf):
    if c.family == "94":
        return D.OS95 if inf["formatSubType"] == 3 else D.OS94
    return OS93[c.version]


def _dropped_93a(c, s):
    """an OS93a stream with every band dropped: the reference encoder writes a header of 0xFF bytes, whose byte 0 the
    decoder reads as Type 1, and the 93a Type-1 band loop then runs past its 18 bands (undefined in the reference: the
    library raises FATAL and stops the frame, as the oracle does)"""
    return c.family == "93a" and s[2:18] == b"\xff" * 16


def test_round_trip_through_the_gpu_decoder(gpu_ctx, oracle, sets, encoded):
    """all bands dropped, masked-shift headers, maximal Type-1 codes: streams the decoder's own tests never make.  The
    GPU decoder's PCM is the oracle's on every stream; its error bits are clear on all but the OS93a all-dropped ones"""
    items = []
    for cases in sets.values():
        for c in cases:
            s, inf = encoded[c.name]
            items.append((c, (_decode_os(c, inf), s, 255, 0x64)))
    batch, frames, n_fatal = [], 0, 0
    for c, item in items + [(None, None)]:
        nf = 0 if item is None else (item[1][0] << 8) | item[1][1]
        if batch and (item is None or frames + nf > 65536):
            got, err, first = gpu_ctx.decode_streams([it for _, it in batch])
            want = np.concatenate([oracle.decode(os_, vol, [s], [lvl], (s[0] << 8) | s[1]) for _, (os_, s, vol, lvl) in batch])
            assert np.array_equal(got, want), [b[0].name for b in batch][:5]
            for k, (bc, (_, s, _, _)) in enumerate(batch):
                e = err[int(first[k]):int(first[k]) + ((s[0] << 8) | s[1])]
                if _dropped_93a(bc, s):
                    assert (e[0] & D.FRAME_FATAL) != 0, bc.name
                    n_fatal += 1
                else:
                    assert not e.any(), (bc.name, np.flatnonzero(e)[:5], e[e != 0][:5])
            batch, frames = [], 0
        if item is not None:
            batch.append((c, item))
            frames += nf
    assert n_fatal > 0
