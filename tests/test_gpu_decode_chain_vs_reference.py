"""The chain decode -> converter -> FLAC writer on the MI355X with nothing of this project's between the expected values and
the reference programs: the expected PCM of dcs_decode_streams_at is the compiled reference decoder's output
(oracle/_ref/libdcsref.so; the C restatement where it is absent) fed through the compiled libsamplerate
(oracle/_ref/dcs_rsout_default), and the bytes of dcs_decode_streams_flac_at must pass the compiled libFLAC's decoder with
MD5 checking against that PCM and equal the writer's restatement of it.  Synthetic streams of all six layouts at 1, 2, 3, 17
and 40 frames, the smallest that give a last block of every P = ctz(n); six rates of tests/rate_out_cases.py."""
import functools
import tempfile

import numpy as np
import pytest

import dcsexplorer_amd as D
import flac_fuzz_cases as Z
import flac_write_any_ref as A
import rate_out_cases as C
from oracle.dcs_oracle import Oracle, Reference, reference_available

pytestmark = pytest.mark.gpu

FRAMES = (1, 2, 3, 17, 40)
EXTRA = 2
# two rates at which the walk is exact, the DCS rate's neighbour, the two people ask for, one seeded draw
RATES = (25600, 64000, 31251, 44100, 48000, C.rates("default")[-1])
assert set(RATES[:2]) <= set(C.dyadic_rates()) and RATES[5] not in RATES[:5]


@functools.lru_cache(maxsize=None)
def streams():
    return [(D.format_os(f), D.synth_stream(f, n, seed=0xC4A1 + 16 * f + i, nbands=18 if f == D.FMT_93A_T1 else 16), 255, 0x64)
            for f in range(6) for i, n in enumerate(FRAMES)]


@functools.lru_cache(maxsize=None)
def decoded():
    """the reference decoder's PCM of every stream, each from a fresh decoder"""
    dec = Reference() if reference_available() else Oracle()
    return [np.ascontiguousarray(dec.decode(os_, vol, [s], [lvl], ((s[0] << 8) | s[1]) + EXTRA), np.int16).ravel()
            for os_, s, vol, lvl in streams()]


@functools.lru_cache(maxsize=None)
def expected(rate):
    """[(int16 samples, nClipped, peak bits)] of every stream at `rate`, by the compiled libsamplerate"""
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for pcm in decoded():
            y, yf = C.reference_convert(pcm, "default", rate, tmp)
            out.append((y, sum(C.clamp_counts(yf)), C.peak_bits(yf)))
    return out


def test_the_last_blocks_have_every_partition_limit():
    """a condition on the reference's output alone"""
    if not C.checker_available():
        pytest.skip(C.MISSING)
    assert [len(p) for p in decoded()] == [240 * (n + EXTRA) for _ in range(6) for n in FRAMES]
    seen = {A.finest(len(y) % A.BLOCK or A.BLOCK) for rate in RATES for y, _, _ in expected(rate)}
    assert seen == {0, 1, 2, 3, 4}, seen
    assert any(len(y) > A.BLOCK for y, _, _ in expected(48000))


@pytest.mark.parametrize("rate", RATES)
def test_decode_at_a_rate_equals_the_reference_programs(gpu_ctx, rate):
    if not C.checker_available():
        pytest.skip(C.MISSING)
    want = expected(rate)
    out, info, err, first = gpu_ctx.decode_streams_at(list(streams()), rate, extra_frames=EXTRA)
    assert len(out) == len(want) and not err.any()
    for k, (y, clipped, peak) in enumerate(want):
        assert np.array_equal(out[k], y), (k, len(out[k]), len(y))
        assert (int(info[k]["nIn"]), int(info[k]["nOut"]), int(info[k]["nClipped"]), int(info[k]["peak"].view(np.uint32))) == (
            len(decoded()[k]), len(y), clipped, peak), k
    for md5 in (True, False):
        flac, winfo, rate_info, ferr, ffirst = gpu_ctx.decode_streams_flac_at(list(streams()), rate, extra_frames=EXTRA, md5=md5)
        assert rate_info.tobytes() == info.tobytes() and np.array_equal(ferr, err) and np.array_equal(ffirst, first)
        for k, (y, _, _) in enumerate(want):
            assert flac[k] == A.write(y, rate, md5)[0], (k, md5, len(y))
        if Z.checker_available():
            assert Z.check_md5([(b, y) for b, (y, _, _) in zip(flac, want)]) == ["ok"] * len(want)
