#!/usr/bin/env python3
"""Generates the output-rate converter's fixtures from the reference's own code (build container only; outputs are data):

  decode_rate_golden.{json,npz}   int16 PCM at 31 250 Hz in, libsamplerate's output at an output rate out, run as
                                  resample/out_rate_driver.c runs it: src_short_to_float_array, the reference encoder's
                                  call pattern at the ratio outRate / 31250.0, src_float_to_short_array.  Inputs are
                                  recipes (decode_rate_ref.case_pcm); per case the count, the sha256 of the int16 output,
                                  the two clamping branches' counts and the bits of the float output's peak, and the
                                  samples of the short cases.  The npz also holds this fixture's own long table, for
                                  which the 512-sample flush cap binds at 44.1 kHz and above (the long table of
                                  resample_filters.npz is too short for that at a ratio of 2 and less).

The converter is built once per table by oracle.rsref.build_lsr, into a temporary directory: the library's default table,
the long table, big_table() of the default one; the vendored fastest and medium tables are the other two slots of the
default build.  Asserted on the reference's output alone: the clip case clamps in both signs at 44 100 and at 48 000, and
the flush cap binds on the long table.
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
import decode_rate_ref as Q     # noqa: E402  (case_pcm: the inputs, kept as recipes)
from oracle.rsref import build_lsr, big_table, npz_table      # noqa: E402
HERE = os.path.join(ROOT, "tests", "golden")
RATES = (4000, 8000, 11025, 22050, 31250, 32000, 44100, 48000, 65535)
KEEP = 400              # cases with at most this many outputs keep their samples
CONV = {"default": 0, "medium": 1, "fastest": 2, "long": 0, "big": 0}
CLIP = "square:4080:0"


def long_table():
    """400 input samples each side: at the end of input more than 512 outputs are still due from 44.1 kHz up"""
    inc, half = 8, 400
    t = np.arange(half * inc + 2) / inc
    fc = 0.85
    c = fc * np.sinc(fc * t) * np.i0(9.0 * np.sqrt(np.clip(1 - (t / half) ** 2, 0, 1))) / np.i0(9.0)
    c[t >= half] = 0.0
    return c.astype(np.float32), inc


def cases():
    """(name, table, recipe, rate)"""
    out = []
    for rate in RATES:
        for n in (1, 15, 16, 17, 240, 480, 4080, 4095, 4096, 4097):
            out.append(("default", "noise:%d:%d" % (n, n + rate), rate))
        for key in (CLIP, "dc+:480:0", "dc-:480:0", "impulse:240:0", "silence:240:0"):
            out.append(("default", key, rate))
    for tab in ("fastest", "medium", "big"):
        for rate in (8000, 44100, 48000):
            for key in ("noise:17:5", "noise:240:6", "noise:4097:7", CLIP):
                out.append((tab, key, rate))
    for rate in (4000, 44100, 48000, 65535):
        for key in ("noise:300:8", "noise:4097:9", "noise:1:10"):
            out.append(("long", key, rate))
    return [("%s-%d-%s" % (t, r, k), t, k, r) for t, k, r in out]


def run(exe, pcm, conv, rate, tmp):
    """the driver on int16 samples -> (int16 output, float32 output)"""
    src, dst, dstf = os.path.join(tmp, "in.s16"), os.path.join(tmp, "out.s16"), os.path.join(tmp, "out.f32")
    np.asarray(pcm, "<i2").tofile(src)
    r = subprocess.run([exe, src, dst, dstf, str(conv), str(rate)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s %d %d: %s" % (exe, conv, rate, r.stderr))
    return np.fromfile(dst, "<i2"), np.fromfile(dstf, "<f4")


def build_all(tmp, tables):
    drv = os.path.join(HERE, "resample", "out_rate_driver.c")
    exes = {k: build_lsr(tmp, "out_" + k, *tables[k], drv) for k in ("default", "long", "big")}
    exes["fastest"] = exes["medium"] = exes["default"]
    return exes


def tables_of(long_tab):
    default = npz_table("default")
    return {"default": default, "fastest": npz_table("fastest"), "medium": npz_table("medium"), "big": big_table(*default),
            "long": long_tab}


def main():
    long_tab = long_table()
    tables = tables_of(long_tab)
    arrays = {"long/coeffs": long_tab[0], "long/increment": np.int32(long_tab[1])}
    meta = []
    with tempfile.TemporaryDirectory() as tmp:
        exes = build_all(tmp, tables)
        for name, tab, key, rate in cases():
            y, yf = run(exes[tab], Q.case_pcm(key), CONV[tab], rate, tmp)
            v = yf.astype(np.float64) * 2147483648.0
            hi, lo = int((v >= 2147483647.0).sum()), int((v <= -2147483648.0).sum())
            assert hi <= int((y == 32767).sum()) and lo <= int((y == -32768).sum())
            if len(y) <= KEEP:
                arrays[name + "/out"] = y
            peak = np.float32(np.max(np.abs(yf))) if len(yf) else np.float32(0)
            meta.append(dict(name=name, table=tab, signal=key, rate=rate, count=len(y), sha256=hashlib.sha256(y.tobytes()).hexdigest(),
                             clippedHigh=hi, clippedLow=lo, peakBits=int(peak.view(np.uint32))))
    by = {c["name"]: c for c in meta}
    for rate in (44100, 48000):
        c = by["default-%d-%s" % (rate, CLIP)]
        assert c["clippedHigh"] > 0 and c["clippedLow"] > 0, c
    # the flush cap binds: a count short of the walk without the cap (every output whose position the end rule admits)
    capped = 0
    for c in meta:
        if c["table"] == "long" and c["rate"] >= 44100 and c["signal"].startswith("noise:4097"):
            free = int(np.floor(4097 * (c["rate"] / 31250.0)))
            assert c["count"] < free - 8, (c, free)
            capped += 1
    assert capped >= 3
    np.savez_compressed(os.path.join(HERE, "decode_rate_golden.npz"), **arrays)
    json.dump(dict(cases=meta, keep=KEEP), open(os.path.join(HERE, "decode_rate_golden.json"), "w"), indent=0)
    print("%d cases, %d with the flush cap binding" % (len(meta), capped))


if __name__ == "__main__":
    sys.exit(main())
