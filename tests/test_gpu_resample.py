"""dcs_resample_streams and dcs_encode_streams_at on the MI355X: bit for bit libsamplerate's output run as the reference
encoder runs it (tests/golden/resample_golden.*) and the numpy restatement (tests/resample_ref.py) on a seeded fuzz; byte
for byte the reference DCSEncoder at other input rates (tests/golden/encode_rate_golden.*); independent of the batch
around a stream; the pass-through at 31 250 Hz; loud on bad input, naming the stream."""
import hashlib
import json
import os

import numpy as np
import pytest

import dcsexplorer_amd as D
import resample_ref as R
from dcsexplorer_amd.api import ERR_BAD_STREAM, ERR_INVALID_ARG

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = np.load(os.path.join(HERE, "golden", "resample_filters.npz"))
RS = json.load(open(os.path.join(HERE, "golden", "resample_golden.json")))
RS_ARR = np.load(os.path.join(HERE, "golden", "resample_golden.npz"))
ENC = json.load(open(os.path.join(HERE, "golden", "encode_rate_golden.json")))
ENC_ARR = np.load(os.path.join(HERE, "golden", "encode_rate_golden.npz"))
TABLES = ("fastest", "medium", "default", "long")
ENC_FMT = {(0x9400, -1, -1): None, (0x9400, 0, 0): D.FMT_94_T0, (0x9400, 1, 3): D.FMT_94_T1_S3, (0x9302, -1, -1): None,
           (0x9301, 0, -1): D.FMT_93_T0}


def table(name):
    return FILTERS[name + "/coeffs"], int(FILTERS[name + "/increment"])


def digest(y):
    return hashlib.sha256(np.asarray(y, "<f4").tobytes()).hexdigest()


def same_bits(a, b):
    return len(a) == len(b) and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("tab", TABLES)
def test_resample_matches_libsamplerate(gpu_ctx, tab):
    cases = [k for k in RS["cases"] if k["table"] == tab]
    got = gpu_ctx.resample_streams([R.fixture_pcm(RS_ARR, k["signal"]) for k in cases], [k["rate"] for k in cases],
                                   [k["channels"] for k in cases], filter=table(tab), at_unity=True)
    for k, y in zip(cases, got):
        assert len(y) == k["count"] and digest(y) == k["sha256"], k["name"]


def test_default_filter_is_the_null_filter(gpu_ctx):
    cases = [k for k in RS["cases"] if k["table"] == "default"][:40]
    got = gpu_ctx.resample_streams([R.fixture_pcm(RS_ARR, k["signal"]) for k in cases], [k["rate"] for k in cases],
                                   [k["channels"] for k in cases], at_unity=True)
    for k, y in zip(cases, got):
        assert digest(y) == k["sha256"], k["name"]


def test_resample_fuzz_against_the_restatement(gpu_ctx):
    rng = np.random.default_rng(0x2E5A)
    rates = [4000, 8000, 11025, 16000, 22050, 24000, 31250, 32000, 44100, 48000, 88200, 96000, 192000, 384000]
    tabs = {k: table(k) for k in TABLES}
    for it in range(200):
        tab = ("fastest", "default", "default", "long", "medium")[it % 5]
        c, inc = tabs[tab]
        n = int(rng.integers(1, 9))
        at_unity = bool(rng.integers(0, 2))
        pcm, rs, chs = [], [], []
        for _ in range(n):
            rate = int(rng.choice(rates)) if rng.random() < 0.8 else int(rng.integers(4000, 384001))
            ch = int(rng.integers(1, 3))
            length = int(rng.integers(1, 40)) if rng.random() < 0.3 else int(rng.integers(40, 2500 if tab != "medium" else 600))
            x = (rng.uniform(-1, 1, length) * rng.choice([1.0, 0.5, 1e-3])).astype(np.float32)
            if rng.random() < 0.1:
                x = np.clip(np.rint(x * 32767), -32768, 32767).astype(np.int16)
            pcm.append(x)
            rs.append(rate)
            chs.append(ch)
        got = gpu_ctx.resample_streams(pcm, rs, chs, filter=(c, inc), at_unity=at_unity)
        for x, rate, ch, y in zip(pcm, rs, chs, got):
            xf = x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x
            want = R.resample(xf, rate, c, inc, ch, R.AT_UNITY if at_unity else 0)
            assert same_bits(y, want), (it, tab, rate, ch, len(x), at_unity)


@pytest.mark.parametrize("version,typ,sub", sorted({(c["version"], c["type"], c["subType"]) for c in ENC["cases"]}))
def test_encode_at_matches_the_reference_encoder(gpu_ctx, version, typ, sub):
    cases = [c for c in ENC["cases"] if (c["version"], c["type"], c["subType"]) == (version, typ, sub)]
    out, info = gpu_ctx.encode_streams_at([R.fixture_pcm(ENC_ARR, c["signal"]) for c in cases], [c["rate"] for c in cases], version,
                                          ENC_FMT[(version, typ, sub)], channels=[c["channels"] for c in cases], at_unity=True)
    for c, s, inf in zip(cases, out, info):
        assert len(s) == c["bytes"] and hashlib.sha256(s).hexdigest() == c["sha256"], c["name"]
        assert inf["nBytes"] == len(s)
        if c["name"] + "/stream" in ENC_ARR.files:
            assert s == ENC_ARR[c["name"] + "/stream"].tobytes()


def test_batch_invariance(gpu_ctx):
    rng = np.random.default_rng(0xBA7C)
    lst = [(0.5 * rng.uniform(-1, 1, int(rng.integers(100, 20000)))).astype(np.float32) for _ in range(9)]
    rates = [44100, 48000, 4000, 384000, 22050, 31250, 8000, 96000, 11025]
    chs = [1, 2, 1, 1, 2, 1, 2, 1, 1]
    together = gpu_ctx.resample_streams(lst, rates, chs)
    enc_together, _ = gpu_ctx.encode_streams_at(lst, rates, channels=chs)
    for i in (0, 4, 8):
        alone = gpu_ctx.resample_streams([lst[i]], [rates[i]], [chs[i]])[0]
        assert same_bits(alone, together[i])
        enc_alone, _ = gpu_ctx.encode_streams_at([lst[i]], [rates[i]], channels=[chs[i]])
        assert enc_alone[0] == enc_together[i]
    rev = gpu_ctx.resample_streams(lst[::-1], rates[::-1], chs[::-1])
    assert all(same_bits(a, b) for a, b in zip(rev[::-1], together))


def test_unity_rate_is_encode_streams(gpu_ctx):
    rng = np.random.default_rng(0x3125)
    lst = [(0.6 * np.sin(np.arange(n) * 0.01 * (k + 1)) + 0.1 * rng.uniform(-1, 1, n)).astype(np.float32)
           for k, n in enumerate((1, 239, 240, 241, 5000, 17000))]
    lst.append(np.clip(rng.integers(-20000, 20000, 3000), -32768, 32767).astype(np.int16))
    for version, fmt in ((0x9400, None), (0x9400, D.FMT_94_T1_S0), (0x9302, None), (0x9301, D.FMT_93_T0)):
        got, ginfo = gpu_ctx.encode_streams_at(lst, 31250, version, fmt)
        if version == 0x9400:
            want, winfo = gpu_ctx.encode_streams(lst, fmt)
        else:
            want, winfo = gpu_ctx.encode93_streams(lst, D.OS93A if version == 0x9301 else D.OS93B, fmt)
        assert got == want and np.array_equal(ginfo, winfo)
    assert all(same_bits(a, b if b.dtype == np.float32 else b.astype(np.float32) / np.float32(32768))
               for a, b in zip(gpu_ctx.resample_streams(lst, 31250), lst))


def _fails(fn, status, *words):
    with pytest.raises(D.DcsError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_errors_name_the_stream(gpu_ctx):
    ok = (0.3 * np.sin(np.arange(3000) * 0.05)).astype(np.float32)
    rs, enc = gpu_ctx.resample_streams, gpu_ctx.encode_streams_at
    for fn in (rs, enc):
        _fails(lambda: fn([ok, ok, ok], [44100, 44100, 3999]), ERR_INVALID_ARG, "stream 2", "rate")
        _fails(lambda: fn([ok, ok], [44100, 400000]), ERR_INVALID_ARG, "stream 1", "rate")
        _fails(lambda: fn([ok, ok], [44100, 44100], channels=[1, 3]), ERR_INVALID_ARG, "stream 1", "channels")
        _fails(lambda: fn([ok, np.zeros(0, np.float32)], [44100, 44100]), ERR_INVALID_ARG, "stream 1", "empty")
        nan = ok.copy()
        nan[100] = np.nan
        _fails(lambda: fn([ok, nan], [48000, 48000]), ERR_BAD_STREAM, "stream 1", "finite")
        inf = ok.copy()
        inf[7] = np.inf
        _fails(lambda: fn([inf, ok], [48000, 48000], channels=2), ERR_BAD_STREAM, "stream 0", "finite")
        c, inc = D.resample_filter_default()
        _fails(lambda: fn([ok], [44100], filter=(c[:64], 128)), ERR_INVALID_ARG, "filter")
        _fails(lambda: fn([ok], [44100], filter=(c, 0)), ERR_INVALID_ARG, "filter")
    # resampling overshoots a full-scale square: the converter passes it on, the encoder refuses it and names the peak
    sq = np.where((np.arange(4000) // 50) & 1, 1.0, -1.0).astype(np.float32)
    y = rs([ok, sq], 44100)[1]
    peak = float(np.abs(y).max())
    assert peak > 1.0
    _fails(lambda: enc([ok, sq], 44100), ERR_BAD_STREAM, "stream 1", "peaks at")
    out, _ = enc([ok, sq * np.float32(0.5)], 44100)
    assert len(out) == 2
    # a stream that resamples to nothing, and one longer than 65 535 frames
    assert len(rs([ok, np.full(3, 0.1, np.float32)], 384000)[1]) == 0
    _fails(lambda: enc([ok, np.full(3, 0.1, np.float32)], 384000), ERR_INVALID_ARG, "stream 1", "no samples")
    big = np.zeros(65535 * 240 + 1, np.float32)
    assert D.resample_count(len(big), 31250) == len(big)
    _fails(lambda: enc([ok, big], [44100, 31250]), ERR_INVALID_ARG, "stream 1", "65 535")
    # the context still works
    out, _ = enc([ok], 44100)
    assert len(out[0]) > 18
