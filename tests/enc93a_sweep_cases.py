"""The long case of the OS93a sweep's tests (test infrastructure): one stream of 2 049 frames, one more than the length from
which a stream that dominates its list is decoded through the host-planned batch when it is measured.  The numpy
restatement (tests/enc93a_ref.py) needs about a minute for it, so what it gives is pinned in
tests/golden/encode93a_sweep_golden.json; run this file to compute that again."""
import hashlib
import json
import os

import numpy as np

import enc93a_ref as A

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "encode93a_sweep_golden.json")
LONG_FRAMES = 2049
LONG_RATES = [64000, 16000]
INFO_KEYS = ("selector", "ladderIndex", "numBands", "frameBits", "budgetBits", "sqErr")


def long_signal():
    rng = np.random.default_rng(0x2049)
    return (rng.standard_normal(240 * LONG_FRAMES) * 0.02).astype(np.float32)


def restate_long(chunk=128):
    """the restated streams of long_signal() at LONG_RATES and the default q: the search a chunk of frames at a time (it is
    per frame), one walk, then a choice and an emit per rate"""
    x = long_signal()
    t = A.targets(A.E.analyse(A.E.frames_of(A.E.to_float(x))))
    parts = [A.search(t[f:f + chunk]) for f in range(0, len(t), chunk)]
    searched = tuple(np.concatenate([p[k] for p in parts]) for k in range(3))
    wk = A.walk(*searched, float(np.float32(A.DEFAULTS["maximumQuantizationError"])))
    out = []
    for rate in LONG_RATES:
        ch = A.choose(wk, rate)
        stream, _ = A.emit(t, wk, ch)
        out.append(dict(targetBitRate=rate, nBytes=len(stream), sha256=hashlib.sha256(stream).hexdigest(),
                        info={k: int(ch[k]) for k in INFO_KEYS}))
    return out


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump(dict(signal="default_rng(0x2049).standard_normal(240 * 2049) * 0.02, float32", cases=restate_long()), f, indent=1)
        f.write("\n")
