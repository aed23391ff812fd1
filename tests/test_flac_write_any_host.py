"""The FLAC writer's format for streams of any length, on the host: the general restatement
(tests/flac_write_any_ref.py) of INTEGRATION.md "Writing FLAC" rules 9 to 11 against the whole-frame restatement
(tests/flac_write_ref.py) where both apply, on the cases of tests/flac_write_any_cases.py against the fixture that
tests/golden/make_flac_write_any_golden.py recorded after the vendored libFLAC had decoded every file with its MD5 check
on, against the compiled libFLAC again where it is built, and the argument check of the calls that take any length."""
import hashlib
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import flac_fuzz_cases as Z
import flac_write_any_cases as C
import flac_write_any_ref as A
import flac_write_cases as W
import flac_write_ref as R
from dcsexplorer_amd.api import ERR_INVALID_ARG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {(c["name"], c["rate"], c["md5"]): c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "flac_write_any_golden.json")))["cases"]}
KINDS = ("nBlocks", "nConstant", "nVerbatim", "nFixed")
MD5 = pytest.mark.parametrize("md5", [True, False], ids=["md5", "nomd5"])


@MD5
def test_general_restatement_is_the_whole_frame_one_on_whole_frames(md5):
    """every case of flac_write_cases.cases(): the same bytes and the same info, so existing files do not change"""
    for name, pcm in W.cases():
        assert A.write(pcm, 31250, md5) == R.write(pcm, 31250, md5), name
    for n in (16, 48, 240, 4080, 4096):
        x = C.make("tone", n)
        a, r = A.choose(x), R.choose(x)
        assert a.pop("P") == 4 and a == r, n


def test_cases_make_every_choice():
    t = C.check_tally()
    assert all(v >= 1 for v in t.values()), t
    lengths = {x.size for _, x in C.cases()}
    assert lengths >= set(range(1, 41)) | {47, 63, 79, 80, 81, 255, 256, 257, 4095, 4097, 4098, 4099, 4100, 4101, 8198, 8216, 12345}
    assert {n % 32 for n in lengths} >= {27, 28, 29, 31}
    assert len(C.ragged()) == 300 and all(1 <= x.size <= 9000 for x in C.ragged())
    # the shortest frame there is, a block of 1 sample (always CONSTANT) at frame number 0: the header's 9 bytes (sync and
    # codes 4, the number 1, the block size 1, the rate 2, CRC-8 1), the subframe's 3 and the CRC-16's 2
    b, info = A.write(np.array([-5], np.int16), 48000, True)
    assert len(b) == 42 + 14 and (info["nConstant"], info["minFrame"], info["maxFrame"]) == (1, 14, 14)


def test_fixture_covers_every_case():
    want = {(n, C.RATE, m) for n in [c[0] for c in C.cases()] + ["ragged300"] for m in (True, False)}
    want |= {(n, r, m) for n, _ in C.subset() for r in C.RATES for m in (True, False)}
    assert set(GOLD) == want and len(C.subset()) >= len(C.SUBSET_LENGTHS) * len(C.KINDS)


@MD5
def test_restatement_hashes_to_fixture(md5):
    for rate, cases in [(C.RATE, C.cases())] + [(r, C.subset()) for r in C.RATES]:
        for name, pcm in cases:
            b, info = A.write(pcm, rate, md5)
            g = GOLD[name, rate, md5]
            assert (hashlib.sha256(b).hexdigest(), len(b)) == (g["sha256"], g["bytes"]), (name, rate)
            assert {k: info[k] for k in KINDS} == {k: g[k] for k in KINDS}, (name, rate)
            assert info["nBytes"] == len(b) <= R.write_bound(pcm.size) and info["nSamples"] == pcm.size
            assert b[26:42] == (hashlib.md5(pcm.astype("<i2").tobytes()).digest() if md5 else bytes(16))
    written = [A.write(p, C.RATE, md5) for p in C.ragged()]
    g = GOLD["ragged300", C.RATE, md5]
    blob = b"".join(w[0] for w in written)
    assert (hashlib.sha256(blob).hexdigest(), len(blob), len(written)) == (g["sha256"], g["bytes"], g["streams"])
    assert {k: sum(w[1][k] for w in written) for k in KINDS} == {k: g[k] for k in KINDS}


@pytest.mark.skipif(not Z.checker_available(), reason=Z.MISSING)
@MD5
def test_compiled_libflac_accepts_every_file(md5):
    """FLAC__stream_decoder with MD5 checking on every case and on the ragged list: no exclusions"""
    streams = [x for _, x in C.cases()] + list(C.ragged())
    verdicts = Z.check_md5([(A.write(x, C.RATE, md5)[0], x) for x in streams])
    assert verdicts == ["ok"] * len(streams), [(k, v) for k, v in enumerate(verdicts) if v != "ok"][:8]
    some = [x for _, x in C.subset()]
    for rate in C.RATES:
        assert Z.check_md5([(A.write(x, rate, md5)[0], x) for x in some]) == ["ok"] * len(some), rate


def test_library_reader_accepts():
    """dcs_flac_parse reports the STREAMINFO that was written, dcs_flac_index finds every frame and its length"""
    for name, pcm in C.cases():
        b, info = A.write(pcm, C.RATE, True)
        p = D.flac_parse(b)
        assert p["status"] == 0, (name, p["reason"])
        assert (p["rate"], p["channels"], p["bitDepth"], p["minBlockSize"], p["maxBlockSize"], p["totalSamples"], p["nFrames"]) \
            == (C.RATE, 1, 16, 4096, 4096, pcm.size, info["nBlocks"]), name
        st, frames = D.flac_index(b)
        assert st == 0 and frames["offset"][-1] + frames["length"][-1] == len(b), name
        assert np.array_equal(frames["blockSize"], np.minimum(4096, pcm.size - frames["firstSample"])), name


def test_samples_check_takes_any_length():
    for lengths in ([1], [241], [4096], [239, 1, 4097]):
        assert D.flac_write_samples_check(lengths, 48000) == (0, 0), lengths
    assert D.flac_write_samples_check([(1 << 36) - 1], 48000) == (0, 0)
    for lengths, bad in (([0], 0), ([1 << 36], 0), ([5, 0, 7], 1), ([5, 7, 1 << 36], 2)):
        assert D.flac_write_samples_check(lengths, 48000) == (ERR_INVALID_ARG, bad), lengths
    for rate in (0, 65536, 1 << 31):
        assert D.flac_write_samples_check([1], rate)[0] == ERR_INVALID_ARG, rate
    for rate in (1, 31250, 65535):
        assert D.flac_write_samples_check([1], rate) == (0, 0)
    for flags in (2, 4, 8, 1 << 31):
        assert D.flac_write_samples_check([1], 48000, flags=flags)[0] == ERR_INVALID_ARG, flags
    assert D.flac_write_samples_check([1], 48000, flags=D.FLAC_MD5) == (0, 0)
    # falling offsets, and more than 2^31 - 1 blocks in all
    L = D.load_library()
    offs = np.array([0, 10, 5], np.uint64)
    assert L.dcs_flac_write_samples_check(offs.ctypes.data, 2, 48000, 0, None) == ERR_INVALID_ARG
    assert D.flac_write_samples_check([(1 << 36) - 1] * 129, 48000)[0] == ERR_INVALID_ARG
    assert D.FLAC_AT_UNITY == 4 and D.FLAC_AT_UNITY not in (D.FLAC_MD5, D.FLAC_SEQUENCE)


def test_whole_frame_check_still_refuses_what_it_refused():
    for lengths, bad in (([239], 0), ([241], 0), ([4096], 0), ([240, 1], 1), ([240, 0], 1)):
        assert D.flac_write_check(lengths) == (ERR_INVALID_ARG, bad), lengths
    for flags in (4, 8, 1 << 31):
        assert D.flac_write_check([240], flags=flags)[0] == ERR_INVALID_ARG, flags
    assert D.flac_write_check([240]) == (0, 0)
