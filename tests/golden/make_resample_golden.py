#!/usr/bin/env python3
"""Generates the resampler's fixtures from the reference's own code (build container only; outputs are data):

  resample_filters.npz        the vendored libsamplerate tables SRC_SINC_FASTEST and SRC_SINC_MEDIUM_QUALITY as float32 with
                              their increments (test data), the library's default table (dcs_resample_filter_default) as
                              the bits it must keep, and a long synthetic table for which the 512-sample flush cap binds
  resample_golden.{json,npz}  PCM in, libsamplerate's output out, run as the reference encoder runs it
                              (resample/rs_driver.c: EncodeFile's stereo downmix, 16-sample src_process calls, a 512-float
                              output buffer, one zero-length end-of-input call); the count and sha256 of every case, the
                              bits of the short ones
  encode_rate_golden.{json,npz}  PCM at other rates in, the reference DCSEncoder's stream out (resample/enc_rate_driver.cpp:
                              EncodeFile's loop over OpenStream(rate) / WriteStream(float) / CloseStream), linked with the
                              real vendored libsamplerate whose best-quality slot holds the library's default table

The vendored libsamplerate lacks high_qual_coeffs.h (the reference lists it as missing), so every build here supplies a
stand-in of ours that puts a table of our choice in the best-quality slot; the other two slots are the vendored tables.
The encoder cases are screened with -fsanitize=bounds,shift,float-cast-overflow as make_encode_golden.py screens its
own: a bounds or float-cast report drops the case.  Everything is compiled into a temporary directory.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resample_ref as R        # noqa: E402  (lcg_signal: the long cases' inputs, kept as a recipe)
from oracle.rsref import build_lsr, stand_in, vendored as _vendored      # noqa: E402  (the recipe `make -C oracle rsref` uses)
HERE = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"
LSR = os.path.join(REF, "libsamplerate", "src")
RATES = (4000, 8000, 11025, 22050, 32000, 44100, 48000, 96000, 384000, 31250)
KEEP = 160              # cases with at most this many outputs keep their bits
CONV = {"default": 0, "medium": 1, "fastest": 2, "long": 0}
ENC_FMTS = {"wild": (0x9400, -1, -1), "T0": (0x9400, 0, 0), "T1s3": (0x9400, 1, 3), "93b": (0x9302, -1, -1), "93a": (0x9301, 0, -1)}


def vendored(name):
    return _vendored(LSR, name)


def long_table():
    """wide enough (80 input samples each side) that at 4 kHz more than 512 outputs fall within its reach of the end"""
    inc, half = 32, 80
    t = np.arange(half * inc + 2) / inc
    fc = 0.8
    c = fc * np.sinc(fc * t) * np.i0(8.0 * np.sqrt(np.clip(1 - (t / half) ** 2, 0, 1))) / np.i0(8.0)
    c[t >= half] = 0.0
    return c.astype(np.float32), inc


def signals():
    rng = np.random.default_rng(0x5A3C)
    s = {}
    for n in (1, 2, 3, 7, 16, 17, 48, 99, 160, 255, 300):
        s["noise%d" % n] = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    t = np.arange(4000)
    s["sines4000"] = (0.4 * np.sin(2 * np.pi * t * 0.013) + 0.3 * np.sin(2 * np.pi * t * 0.31)).astype(np.float32)
    s["noise3001"] = rng.uniform(-0.8, 0.8, 3001).astype(np.float32)
    s["square2500"] = np.where((t[:2500] // 37) & 1, 1.0, -1.0).astype(np.float32)
    imp = np.zeros(200, np.float32)
    imp[0] = 1.0
    s["impulse_first"] = imp
    imp = np.zeros(200, np.float32)
    imp[-1] = -1.0
    s["impulse_last"] = imp
    s["silence500"] = np.zeros(500, np.float32)
    return s


def resample_cases(sig):
    """(name, table, signal, rate, channels)"""
    out = []
    short = ["noise1", "noise2", "noise3", "noise7", "noise16", "noise17", "noise48", "noise99", "noise160", "noise255", "noise300"]
    for tab in ("fastest", "medium", "default"):
        for rate in RATES:
            keys = short + ["impulse_first", "impulse_last", "silence500", "sines4000", "noise3001", "square2500"]
            for k in keys:
                out.append(("%s-%d-%s-m" % (tab, rate, k), tab, k, rate, 1))
            for k in ("noise17", "noise300", "sines4000", "square2500"):
                out.append(("%s-%d-%s-s" % (tab, rate, k), tab, k, rate, 2))
    for rate in (4000, 8000, 44100):
        for k in ("noise300", "impulse_last", "noise3001"):
            out.append(("long-%d-%s-m" % (rate, k), "long", k, rate, 1))
    # whole seconds of real rates: the end rule's f64 sum in the converter's buffer indices (sha256 only; the input is a recipe)
    for tab, n, rate, ch in (("default", 441000, 44100, 1), ("default", 882000, 44100, 1), ("default", 576000, 48000, 1),
                             ("default", 640000, 32000, 1), ("default", 882001, 44100, 2), ("fastest", 441000, 44100, 1),
                             ("medium", 96000, 48000, 1), ("long", 160000, 16000, 1)):
        key = "lcg:%d:%d:0.5" % (n, n)
        out.append(("%s-%d-%s-%s" % (tab, rate, key, "s" if ch == 2 else "m"), tab, key, rate, ch))
    return out


def pcm_of(sig, key):
    """a stored signal, or an lcg:<seed>:<n>:<amp> recipe"""
    return R.fixture_pcm({k + "/pcm": v for k, v in sig.items()}, key)


def run(exe, x, args, tmp):
    src, dst = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.f32")
    x.astype("<f4").tofile(src)
    r = subprocess.run([exe, src, dst] + [str(a) for a in args], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s %s: %s" % (exe, args, r.stderr))
    return open(dst, "rb").read(), r.stderr


def encode_cases():
    """(name, signal, rate, channels, fmt)"""
    out = []
    for rate in RATES:
        for fk in ENC_FMTS:
            out.append(("music-%d-%s" % (rate, fk), "music", rate, 1, fk))
        out.append(("stereo-%d-wild" % rate, "stereo", rate, 2, "wild"))
    for fk in ("wild", "93b"):
        out.append(("short-44100-%s" % fk, "short", 44100, 1, fk))
        out.append(("short-4000-%s" % fk, "short", 4000, 1, fk))
    # ten whole seconds at 44.1 and 48 kHz, where the end rule's rounding in the converter's buffer indices decides the count
    out.append(("lcg10s-44100-wild", "lcg:441000:441000:0.5", 44100, 1, "wild"))
    out.append(("lcg10s-48000-93b", "lcg:480000:480000:0.5", 48000, 1, "93b"))
    return out


def enc_signals():
    rng = np.random.default_rng(0xE5A7)
    n = 24000
    t = np.arange(n) / 44100.0
    music = (0.30 * np.sin(2 * np.pi * 440 * t) + 0.15 * np.sin(2 * np.pi * 1250 * t + 1) + 0.05 * rng.standard_normal(n)) \
        * (0.5 + 0.4 * np.sin(2 * np.pi * 3 * t))
    st = np.empty(2 * n + 1, np.float64)
    st[0:2 * n:2] = 0.35 * np.sin(2 * np.pi * 330 * t) + 0.04 * rng.standard_normal(n)
    st[1:2 * n:2] = 0.30 * np.sin(2 * np.pi * 660 * t + 0.3) + 0.04 * rng.standard_normal(n)
    st[-1] = 0.25
    return {"music": music.astype(np.float32), "stereo": st.astype(np.float32),
            "short": (0.4 * rng.uniform(-1, 1, 700)).astype(np.float32)}


def main():
    import dcsexplorer_amd as D
    fastest, medium = vendored("fastest_coeffs.h"), vendored("mid_qual_coeffs.h")
    default = D.resample_filter_default()
    tables = {"fastest": fastest, "medium": medium, "default": default, "long": long_table()}
    np.savez_compressed(os.path.join(HERE, "resample_filters.npz"),
                        **{"%s/coeffs" % k: v[0] for k, v in tables.items()},
                        **{"%s/increment" % k: np.int32(v[1]) for k, v in tables.items()})
    sig = signals()
    arrays = {"%s/pcm" % k: v for k, v in sig.items()}
    meta = []
    with tempfile.TemporaryDirectory() as tmp:
        drv = os.path.join(HERE, "resample", "rs_driver.c")
        exes = {"default": build_lsr(tmp, "default", *default, drv), "long": build_lsr(tmp, "long", *tables["long"], drv)}
        exes["fastest"] = exes["medium"] = exes["default"]
        for name, tab, key, rate, ch in resample_cases(sig):
            out, _ = run(exes[tab], pcm_of(sig, key), [CONV[tab], rate, ch], tmp)
            y = np.frombuffer(out, "<f4")
            if len(y) <= KEEP:
                arrays[name + "/out"] = y
            meta.append(dict(name=name, table=tab, signal=key, rate=rate, channels=ch, count=len(y),
                             sha256=hashlib.sha256(out).hexdigest()))
        n_capped = sum(1 for c in meta if c["table"] == "long" and c["rate"] == 4000)
        print("%d resample cases (%d on the long table at 4 kHz)" % (len(meta), n_capped))
        np.savez_compressed(os.path.join(HERE, "resample_golden.npz"), **arrays)
        json.dump(dict(cases=meta, keep=KEEP), open(os.path.join(HERE, "resample_golden.json"), "w"), indent=0)

        # the reference encoder over the real converter, the default table in the best-quality slot
        edrv = os.path.join(HERE, "resample", "enc_rate_driver.cpp")
        enc = build_lsr(tmp, "enc", *default, edrv, cxx=True)
        san = build_lsr(tmp, "encsan", *default, edrv, cxx=True, extra=["-fsanitize=bounds,shift,float-cast-overflow"])
        es = enc_signals()
        earr = {"%s/pcm" % k: v for k, v in es.items()}
        emeta, dropped = [], []
        for name, key, rate, ch, fk in encode_cases():
            fv, typ, sub = ENC_FMTS[fk]
            args = [rate, ch, "%x" % fv, typ, sub]
            _, report = run(san, pcm_of(es, key), args, tmp)
            kinds = sorted({("shift" if "shift" in l else "bounds" if "out of bounds" in l or "index" in l else "float-cast")
                            for l in report.splitlines() if "runtime error" in l})
            if any(k != "shift" for k in kinds):
                dropped.append(dict(name=name, ubsan=kinds))
                continue
            stream, _ = run(enc, pcm_of(es, key), args, tmp)
            if len(stream) <= 2048:
                earr[name + "/stream"] = np.frombuffer(stream, np.uint8)
            emeta.append(dict(name=name, signal=key, rate=rate, channels=ch, fmt=fk, version=fv, type=typ, subType=sub,
                              bytes=len(stream), sha256=hashlib.sha256(stream).hexdigest(), ubsan=kinds))
        np.savez_compressed(os.path.join(HERE, "encode_rate_golden.npz"), **earr)
        json.dump(dict(cases=emeta, dropped=dropped), open(os.path.join(HERE, "encode_rate_golden.json"), "w"), indent=0)
        print("%d encode cases, %d dropped: %s" % (len(emeta), len(dropped), dropped))


if __name__ == "__main__":
    sys.exit(main())
