"""Writes tests/golden/encode93a_fuzz_golden.json: sizes, FNV-1a hashes and the choice of some twenty streams of the numpy
restatement of the OS93a Type-1 encoder (tests/enc93a_ref.py) on the seeded cases of tests/enc93a_fuzz_cases.py, spread over
their kinds and the large maximumQuantizationError values.  tests/test_encode93a_vs_reference.py checks the restatement
there against the compiled reference decoder; the file pins it: a change to it that the kernels follow shows here."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import enc93a_fuzz_cases as Z  # noqa: E402

# a case at its set's rate and q (None), at the top rate, or at a rate and q of its own
PICK = [("quiet/noise_peak1", "top"), ("quiet/noise_peak2", None), ("quiet/tone_peak2", None), ("quiet/noise_peak8", "top"), ("one_band/00", "top"),
        ("one_band/09", None), ("one_band/17", None), ("gaps/interleaved", None), ("gaps/lonely", None), ("gaps/every17", None),
        ("ramp/steps", None), ("full_scale/square_half1", "top"), ("full_scale/dc", None), ("long/256", None), ("long/257", None),
        ("full_scale/sine_word100", (128000, 12000.0)), ("gaps/every17", (Z.TOP_RATE, 18000.0)),
        ("one_band/13", (64000, 3.4028234663852886e+38)), ("s33/0/unit/479", (Z.TOP_RATE, Z.Q_NEAR_2_64)),
        ("full_scale/dc", (128000, 1.0))]
PICK += [(n, None) for n in Z.NAMES if n.startswith("low_prv/")]

if __name__ == "__main__":
    out = []
    for name, how in PICK:
        c = Z.CASES[name]
        rate, q = (c.rate, c.q) if how is None else (Z.TOP_RATE, c.q) if how == "top" else how
        s, ch, _ = Z.type1(name, rate, q)
        out.append(dict(signal=name, rate=rate, mqe=q, bytes=len(s), fnv1a64="%016x" % Z.fnv1a64(s),
                        info=[ch[k] for k in ("selector", "ladderIndex", "numBands", "frameBits", "sqErr")]))
    with open(os.path.join(HERE, "encode93a_fuzz_golden.json"), "w") as f:
        json.dump(dict(streams=out), f, indent=1)
        f.write("\n")
    print(len(out), "streams")
