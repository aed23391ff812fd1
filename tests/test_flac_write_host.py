"""The FLAC writer's format on the host: the numpy restatement (tests/flac_write_ref.py) of INTEGRATION.md "Writing FLAC"
on the cases of tests/flac_write_cases.py, against the fixture that tests/golden/make_flac_write_golden.py recorded after
the vendored libFLAC had decoded every file with its MD5 check on; the library's own FLAC reader (dcs_flac_parse,
dcs_flac_index) and its Python restatement (tests/flac_ref.py) on the same files; the bound; the argument check."""
import hashlib
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import flac_ref as FR
import flac_write_cases as C
import flac_write_ref as R
from dcsexplorer_amd.api import ERR_INVALID_ARG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {(c["name"], c["md5"]): c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "flac_write_golden.json")))["cases"]}
NAMES = [name for name, _ in C.cases()]
KINDS = ("nBlocks", "nConstant", "nVerbatim", "nFixed")


@pytest.fixture(scope="module")
def written():
    return {(name, md5): R.write(pcm, 31250, md5) for name, pcm in C.cases() for md5 in (True, False)}


def test_fixture_covers_every_case():
    assert set(GOLD) == {(n, m) for n in NAMES + [s[0] for s in C.shapes()] for m in (True, False)}


@pytest.mark.parametrize("md5", [True, False], ids=["md5", "nomd5"])
def test_restatement_hashes_to_fixture(written, md5):
    for name in NAMES:
        b, info = written[name, md5]
        g = GOLD[name, md5]
        assert (hashlib.sha256(b).hexdigest(), len(b)) == (g["sha256"], g["bytes"]), name
        assert {k: info[k] for k in KINDS} == {k: g[k] for k in KINDS}, name
        assert info["nBytes"] == len(b) and info["nSamples"] == dict(C.cases())[name].size
    for name, pool, index in C.shapes():
        ref = [R.write(p, 31250, md5) for p in pool]
        g = GOLD[name, md5]
        h = hashlib.sha256()
        for i in index:
            h.update(ref[i][0])
        assert (h.hexdigest(), sum(len(ref[i][0]) for i in index), len(index)) == (g["sha256"], g["bytes"], g["streams"]), name
        assert {k: sum(ref[i][1][k] for i in index) for k in KINDS} == {k: g[k] for k in KINDS}, name


def test_cases_reach_what_they_are_for(written):
    """the kinds, orders and header forms the case list is there to exercise"""
    kinds = lambda name: tuple(written[name, True][1][k] for k in KINDS[1:])
    assert kinds("silence") == (3, 0, 0) and kinds("const_min") == (3, 0, 0)
    assert kinds("alternating") == (0, 3, 0) and kinds("white") == (0, 3, 0)
    pcm = dict(C.cases())
    assert R.choose(pcm["noise3"][:4096])["order"] == 0 and max(R.choose(pcm["noise3"][:4096])["k"]) <= 2
    ramp = R.choose(pcm["ramp"][:4096])
    assert (ramp["order"], ramp["p"], ramp["k"]) == (2, 0, [0])
    assert R.choose(pcm["spike"][4096:8192])["p"] >= 3
    assert R.frame_header(0, 240, 31250)[2] >> 4 == 0x6 and R.frame_header(0, 4080, 31250)[2] >> 4 == 0x7
    assert [len(R.utf8(v)) for v in (127, 128, 2047, 2048, 65535, 65536, (1 << 36) - 1)] == [1, 2, 2, 3, 3, 4, 7]
    assert written["len2200", True][1]["nBlocks"] > 128 and written["len35000", True][1]["nBlocks"] > 2048


def test_short_last_blocks_reach_the_partition_rule(written):
    """blocks of 16, 32 and 48 samples: predictor orders 1..4 occur at each length, no written partition is as short as the
    warm-up, the first partition's parameter is there (the bit count matches), and at each length some tail would take a
    forbidden partition order if the rule were not applied"""
    pcm = dict(C.cases())
    for frames, n, seeds in C.SHORT_TAILS:
        orders, binds = set(), 0
        for kind, ss in seeds.items():
            for seed in ss:
                tail = pcm["tail%d_%d_%d" % (n, kind, seed)][-n:]
                assert tail.size == n == (frames * 240) % 4096
                c, free = R.choose(tail), R.choose(tail, constrain=False)
                assert c["kind"] == R.FIXED and (n >> c["p"]) > c["order"] and len(c["k"]) == 1 << c["p"]
                body = R.subframe(tail)[1]
                assert len(body) == (8 + c["bits"] + 7) // 8
                orders.add(c["order"])
                binds += free["kind"] == R.FIXED and (n >> free["p"]) <= free["order"]
        assert orders >= {1, 2, 3, 4} and binds >= 1, (n, orders, binds)
    square = R.choose(pcm["tail16_square"][-16:])
    assert (square["kind"], square["order"]) == (R.FIXED, 1) and (16 >> square["p"]) > 1


def test_crc16_by_parts_is_the_serial_crc16(written):
    b = written["white", True][0]
    for length in (64, 65, 1000, 8209):
        assert R.crc16(b[42:42 + length]) == R.crc16_serial(b[42:42 + length])


@pytest.mark.parametrize("name", NAMES)
def test_flac_ref_decodes_to_the_source(written, name):
    pcm = dict(C.cases())[name]
    for md5 in (True, False):
        b = written[name, md5][0]
        st, ints, info = FR.integers(b)
        assert st == FR.OK, info
        assert np.array_equal(ints, pcm.astype(np.int64))
        assert b[26:42] == (hashlib.md5(pcm.astype("<i2").tobytes()).digest() if md5 else bytes(16))
        if name == "len35000":
            break                                       # (the frames are the same without the MD5: one walk of 8.4 M samples)


@pytest.mark.parametrize("name", NAMES)
def test_library_reader_accepts(written, name):
    """dcs_flac_parse reports the STREAMINFO that was written, dcs_flac_index finds every frame"""
    pcm = dict(C.cases())[name]
    b, info = written[name, True]
    p = D.flac_parse(b)
    assert p["status"] == 0, p["reason"]
    assert (p["rate"], p["channels"], p["bitDepth"], p["minBlockSize"], p["maxBlockSize"], p["totalSamples"], p["firstFrameOffset"]) \
        == (31250, 1, 16, 4096, 4096, pcm.size, 42)
    assert p["nFrames"] == info["nBlocks"]
    assert (int.from_bytes(b[12:15], "big"), int.from_bytes(b[15:18], "big")) == (info["minFrame"], info["maxFrame"])
    st, frames = D.flac_index(b)
    assert st == 0 and frames.size == info["nBlocks"]
    assert frames["offset"][0] == 42 and np.array_equal(frames["offset"][1:], (frames["offset"] + frames["length"])[:-1])
    assert frames["offset"][-1] + frames["length"][-1] == len(b)
    assert np.array_equal(frames["firstSample"], np.arange(frames.size) * 4096)
    assert np.array_equal(frames["blockSize"], np.minimum(4096, pcm.size - frames["firstSample"]))
    assert (frames["length"].min(), frames["length"].max()) == (info["minFrame"], info["maxFrame"])


def test_bound(written):
    for name, pcm in C.cases():
        assert D.flac_write_bound(pcm.size) == R.write_bound(pcm.size) >= len(written[name, True][0])
    assert D.flac_write_bound(240) == 42 + 8211 and D.flac_write_bound(4097) == 42 + 2 * 8211
    # the VERBATIM fallback is what makes it a bound: noise costs a header, the subframe's byte, the samples and the CRC-16
    assert len(written["white", True][0]) == 42 + 2 * (8 + 1 + 2 * 4096 + 2) + (9 + 1 + 2 * 208 + 2)


def test_argument_check():
    ok = D.flac_write_check([240, 480, 240 * 300])
    assert ok == (0, 0)
    for lengths, bad in (([240, 241], 1), ([239], 0), ([240, 0, 240], 1), ([480, 240, 4096], 2), ([240, 1 << 36], 1)):
        assert D.flac_write_check(lengths) == (ERR_INVALID_ARG, bad), lengths
    assert D.flac_write_check([((1 << 36) - 1) // 240 * 240]) == (0, 0)
    for rate in (0, 65536, 1 << 31):
        assert D.flac_write_check([240], rate=rate)[0] == ERR_INVALID_ARG, rate
    for rate in (1, 31250, 65535):
        assert D.flac_write_check([240], rate=rate) == (0, 0)
    assert D.flac_write_check([240], flags=4)[0] == ERR_INVALID_ARG
    assert D.flac_write_check([240], flags=D.FLAC_MD5) == (0, 0)
