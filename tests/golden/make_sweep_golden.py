#!/usr/bin/env python3
"""Generates tests/golden/sweep_golden.json: for the four rec* recordings of encode_golden.npz at six bit rates (wildcard
layout, every other parameter at the reference's default), what the COMPILED REFERENCE makes of them: the stream of
oracle/_ref/dcs_encref (length, SHA-256, the layout written), and that stream decoded by oracle/_ref/libdcsref.so as a fresh
decoder at volume, mixing level 0xFF for nFrames + 1 frames, compared with its source as dcs_encode_sweep's
DCS_SWEEP_MEASURE defines it (tests/sweep_ref.py): nCompared, sumSrcSq, sumDecSq, sumCross, peakErr at lag 16, and the
squared error at every lag 0..255 (the test asserts that 16 is the smallest).  Recorded results only.

Build container only (needs oracle/_ref, made by `make -C oracle ref` where the reference sources are mounted)."""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import sweep_ref                                                    # noqa: E402
from make_encode_golden import DEFAULTS, build, run                 # noqa: E402
from oracle.dcs_oracle import Reference                             # noqa: E402

OS94, OS95 = 2, 3


def main():
    arr = np.load(os.path.join(ROOT, "tests", "golden", "encode_golden.npz"))
    ref = Reference()
    cases = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(False)
        for v in range(4):
            x = arr["rec%d/pcm" % v]
            for rate in sweep_ref.RATES:
                stream, _ = run(exe, x, "wild", dict(DEFAULTS, targetBitRate=rate), tmp)
                n_frames = (stream[0] << 8) | stream[1]
                typ, sub = stream[2] >> 7, ((stream[3] >> 7) << 1) | (stream[4] >> 7)
                dec = ref.decode(OS95 if sub == 3 else OS94, 255, [stream], [255], n_frames + 1)
                m = sweep_ref.measure(x, dec)
                q = sweep_ref.quantise(x)
                d = dec.reshape(-1).astype(np.int64)
                lags = []
                for lag in range(256):
                    dd = np.zeros(len(q), np.int64)
                    have = max(0, min(len(q), len(d) - lag))
                    dd[:have] = d[lag:lag + have]
                    lags.append(int(((dd - q) ** 2).sum()))
                cases.append(dict(signal="rec%d" % v, targetBitRate=rate, winner=[typ, sub], nFrames=n_frames, bytes=len(stream),
                                  sha256=hashlib.sha256(stream).hexdigest(), sqErrAtLag=lags, **m))
                print(cases[-1]["signal"], rate, len(stream), sweep_ref.sq_err(m), int(np.argmin(lags)))
    with open(os.path.join(ROOT, "tests", "golden", "sweep_golden.json"), "w") as f:
        json.dump(dict(cases=cases), f, indent=None, separators=(",", ":"))


if __name__ == "__main__":
    sys.exit(main())
