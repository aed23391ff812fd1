"""Writes tests/golden/encode93a_golden.json: sizes, FNV-1a hashes and the choice of a dozen streams of the numpy
restatement of the OS93a Type-1 encoder (tests/enc93a_ref.py), checked there against the compiled reference decoder by
tests/test_encode93a_host.py.  The file pins the restatement: a change to it that the kernels follow shows here."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import enc93a_cases as C  # noqa: E402

PICK = [("sine100_fs", 8000, 0.0), ("sine100_fs", 128000, 10 / 32768), ("noise_fs", 8000, 0.0), ("noise_fs", 128000, 0.0),
        ("noise_fs", 1000000, 10 / 32768), ("tone_band17", 64000, 0.0), ("noise_m60", 128000, 0.0), ("dc", 64000, 10 / 32768),
        ("len1", 128000, 0.0), ("len241", 64000, 0.0), ("len481", 1000000, 0.0), ("silence", 128000, 0.0)]
PICK += [(n, 128000, 10 / 32768) for n in C.NAMES if n.startswith("rec:")][:4]

if __name__ == "__main__":
    out = []
    for name, rate, mqe in PICK:
        s, ch, _ = C.type1(name, rate, mqe)
        out.append(dict(signal=name, rate=rate, mqe=mqe, bytes=len(s), fnv1a64="%016x" % C.fnv1a64(s),
                        info=[ch[k] for k in ("selector", "ladderIndex", "numBands", "frameBits", "sqErr")]))
    json.dump(dict(streams=out), open(os.path.join(HERE, "encode93a_golden.json"), "w"), indent=1)
    print(len(out), "streams")
