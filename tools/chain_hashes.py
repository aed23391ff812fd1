#!/usr/bin/env python3
"""What the converter-to-encoder entry points produce, as digests: a fixed, seeded list of calls through
dcs_encode_streams_at(_level), dcs_resample_streams_level, dcs_level_streams and dcs_encode_files(_level)
(tests/chain_calls.py makes the calls with every output buffer pre-filled).  One line per call: its name, the status, and
the first 16 hex digits of SHA-256 of the dcs_last_error text, the output buffer, the offsets, the info array and the level
info array, each as the library left it (a refused call's untouched buffers included).

Run it once per build (DCS_HIP_LIB names the other one) and compare: a change that leaves behaviour alone gives the same
lines.  `--join a.txt b.txt` prints two such outputs side by side, with a last column that says whether the lines agree.
Reads neither the reference nor the oracle; the host-walk call apart, inputs are a few thousand samples."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dcsexplorer_amd as D                     # noqa: E402
from dcsexplorer_amd.api import LEVEL_CLIP, LEVEL_FIT, LEVEL_GAIN, LEVEL_NORMALIZE, Level      # noqa: E402

F32 = np.float32


def digest(x):
    if x is None:
        return "-" * 16
    b = x.encode() if isinstance(x, str) else np.ascontiguousarray(x).tobytes()
    return hashlib.sha256(b).hexdigest()[:16]


def levels():
    """(name, level): none, every mode with and without the clamp; a list of them is one level per stream"""
    out = [("none", None)]
    for mode, name, gain, ceiling in ((LEVEL_GAIN, "gain0.5", 0.5, 1.0), (LEVEL_GAIN, "gain1.5c0.9", 1.5, 0.9), (LEVEL_FIT, "fit", 1.0, 1.0),
                                      (LEVEL_FIT, "fit0.5", 1.0, 0.5), (LEVEL_NORMALIZE, "norm0.89", 1.0, 0.8912509)):
        for flags in (0, LEVEL_CLIP):
            out.append(("%s%s" % (name, "+clip" if flags else ""), Level(mode, flags, gain, ceiling)))
    return out


def per_stream(n):
    ls = [Level(LEVEL_FIT, 0, 1.0, 0.8912509), Level(LEVEL_NORMALIZE, 0, 1.0, 1.0), Level(LEVEL_GAIN, LEVEL_CLIP, 1.25, 0.9),
          Level(LEVEL_GAIN, 0, 0.5, 1.0), Level(LEVEL_FIT, LEVEL_CLIP, 1.0, 0.5), Level(LEVEL_NORMALIZE, LEVEL_CLIP, 1.0, 0.25)]
    return [ls[i % len(ls)] for i in range(n)]


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--join":
        a, b = (open(p).read().splitlines() for p in sys.argv[2:4])
        same = len(a) == len(b)
        for i in range(max(len(a), len(b))):
            x, y = (a[i] if i < len(a) else ""), (b[i] if i < len(b) else "")
            same = same and x == y
            print("%s | %s | %s" % (x, y.split(" ", 1)[1] if " " in y else y, "same" if x == y else "DIFFERENT"))
        print("# %d calls, %s" % (len(a), "every line the same" if same else "DIFFERENCES"))
        return 0 if same else 1

    import chain_calls as C
    import flac_cases as FC
    import wav_cases as WC

    rng = np.random.default_rng(0xC4A1)
    sq = np.where((np.arange(1200) // 50) & 1, -1.0, 1.0).astype(F32)
    noise = rng.uniform(-0.4, 0.4, 500).astype(F32)
    quiet = (0.3 * np.sin(np.arange(3000) * 0.05)).astype(F32)
    nan = quiet.copy()
    nan[100] = np.nan
    tiny = np.full(3, 0.1, F32)
    pcm16 = rng.integers(-20000, 20000, 2500).astype(np.int16)
    # loud and quiet streams, mono and stereo, a pass-through rate
    loud = ([np.repeat(sq, 2), noise, sq[:700] * F32(0.95), sq, pcm16], [44100, 8000, 31250, 48000, 22050], [2, 1, 1, 1, 1])
    soft = ([np.repeat(quiet, 2) * F32(0.9), noise, sq[:700] * F32(0.95), pcm16], [44100, 8000, 31250, 11025], [2, 1, 1, 2])
    ctx = D.Context(0)
    calls = []

    def run(name, c):
        calls.append(name)
        print("%-58s %3d %s %s %s %s %s" % (name, c.status, digest(c.msg), digest(c.out), digest(c.offs), digest(c.info), digest(c.linfo)))

    # ------------------------------------------------------------------------------------------------------- streams
    for version in (0x9400, 0x9302, 0x9301):
        for lname, level in levels() + [("per_stream", None)]:
            for at_unity in (False, True):
                for sname, (pcm, rates, chans) in (("loud", loud), ("soft", soft)):
                    lv = per_stream(len(pcm)) if lname == "per_stream" else level
                    if version != 0x9400 and (at_unity or (lname.endswith("+clip") and sname == "soft")):
                        continue                # (the OS93 encoders: a thinner sample of the same grid)
                    run("enc_at %x %s %s%s" % (version, lname, sname, " unity" if at_unity else ""),
                        C.enc_at(ctx, pcm, rates, version, channels=chans, at_unity=at_unity, level=lv))
    run("enc_at 9400 T1S0 soft", C.enc_at(ctx, *soft[:2], 0x9400, D.FMT_94_T1_S0, channels=soft[2]))
    run("enc_at 9301 T0 soft fit", C.enc_at(ctx, *soft[:2], 0x9301, D.FMT_93_T0, channels=soft[2], level=Level(LEVEL_FIT)))
    for lname, level in levels() + [("per_stream", per_stream(5))]:
        for at_unity in (False, True):
            run("resample %s%s" % (lname, " unity" if at_unity else ""), C.resample(ctx, *loud[:2], loud[2], at_unity=at_unity, level=level))
        if level is not None:
            lens = [0, 1, 3, 239, 241, 4097]
            sig = [rng.uniform(-1.3, 1.3, n).astype(F32) for n in lens]
            run("level_streams %s" % lname, C.level_streams(ctx, sig[:5] if lname == "per_stream" else sig, level))
    # the refusals, and what they leave behind
    fit, unit = Level(LEVEL_FIT), Level(LEVEL_GAIN, gain=1.0)
    for lname, level in (("none", None), ("gain1", unit), ("fit", fit)):
        run("refuse enc_at sq,tiny %s" % lname, C.enc_at(ctx, [sq, tiny], [44100, 384000], level=level))
        run("refuse enc_at tiny,sq %s" % lname, C.enc_at(ctx, [tiny, sq], [384000, 44100], level=level))
        run("refuse enc_at tiny,nan %s" % lname, C.enc_at(ctx, [tiny, nan], [384000, 48000], level=level))
        run("refuse enc_at 9302 sq,tiny %s" % lname, C.enc_at(ctx, [sq, tiny], [44100, 384000], 0x9302, level=level))
        run("refuse resample ok,nan short %s" % lname, C.resample(ctx, [quiet, nan], [48000, 48000], level=level, short=1))
        run("refuse resample short %s" % lname, C.resample(ctx, [sq, quiet], [44100, 48000], level=level, short=1))
        run("resample empty %s" % lname, C.resample(ctx, [], [], level=level))
        run("enc_at empty %s" % lname, C.enc_at(ctx, [], [], level=level))
        run("refuse enc_at empty stream %s" % lname, C.enc_at(ctx, [quiet, np.zeros(0, F32)], 44100, level=level))
    bad = [Level(7), fit]
    run("refuse enc_at rate+level", C.enc_at(ctx, [quiet, quiet], [44100, 3999], level=bad))
    run("refuse enc_at level", C.enc_at(ctx, [quiet, quiet], 44100, level=bad))
    run("refuse enc_at levels count", C.enc_at(ctx, [quiet, quiet, quiet], 44100, level=((Level * 2)(fit, fit), 2)))
    run("refuse enc_at levels null", C.enc_at(ctx, [quiet], 44100, level=(None, 1)))
    run("refuse enc_at type1+rate", C.enc_at(ctx, [quiet, quiet], [44100, 3999], 0x9301, level=bad, streamFormatType=1))
    run("refuse enc_at params+rate", C.enc_at(ctx, [quiet, quiet], [44100, 3999], level=bad, targetBitRate=0))
    run("refuse enc_at gain1.5", C.enc_at(ctx, [noise, sq[:700] * F32(0.95)], [8000, 31250], level=Level(LEVEL_GAIN, gain=1.5)))
    run("refuse resample overflow", C.resample(ctx, [quiet, np.full(900, 3e38, F32)], 31250, level=Level(LEVEL_GAIN, gain=2.0)))
    run("refuse resample level", C.resample(ctx, [quiet, quiet], 44100, level=bad))
    run("refuse resample clip short", C.resample(ctx, [sq, quiet], [44100, 48000], level=Level(LEVEL_GAIN, LEVEL_CLIP, 1.0, 1.0), short=1))
    run("refuse level_streams short nan", C.level_streams(ctx, [quiet, nan], fit, short=1))
    run("refuse level_streams nan", C.level_streams(ctx, [quiet, nan], fit))
    run("refuse level_streams overflow", C.level_streams(ctx, [quiet, np.full(3, 3e38, F32)], Level(LEVEL_GAIN, gain=2.0)))
    run("refuse level_streams level", C.level_streams(ctx, [quiet, quiet], bad))
    run("level_streams empty", C.level_streams(ctx, [], fit))
    # --------------------------------------------------------------------------------------------------------- files
    wav, flac = dict(WC.cases()), dict(FC.cases())

    def dcsa(fmt, frames, seed):
        s = D.synth_stream(fmt, frames, seed=seed)
        return D.dcsa_header(D.format_os(fmt), len(s)) + s

    every_format = [wav[k] for k in ("u8_1ch_8000", "u8_2ch_44100", "s16_1ch_22050", "s16_2ch_48000", "s24_1ch_31250", "s24_2ch_22050",
                                     "s32_1ch_44100", "s32_2ch_8000", "f32_1ch_48000", "f32_2ch_31250", "f64_1ch_22050", "f64_2ch_44100",
                                     "ima_256_1ch", "ima_512_2ch", "ima_partial_block", "ext_float_f32", "odd_chunk_pad")]
    flacs = [flac[k] for k in ("types_s16_mono", "rice_s24_mono", "wasted_s16_stereo", "assign_s8_stereo", "block_sizes_variable_mono",
                               "stereo_odd_total", "fullscale_s16_31250", "fullscale_s8_31250")]
    boxes = [dcsa(D.FMT_94_T0, 10, 3), dcsa(D.FMT_94_T1_S0, 12, 4), dcsa(D.FMT_93_T0, 9, 5)]
    mixed = [every_format[2], boxes[0], flacs[6], wav["fullscale_s16_31250"], boxes[2], every_format[12], flacs[2], wav["fullscale_u8_31250"]]
    for version in (0x9400, 0x9302, 0x9301):
        for at_unity in (False, True):
            run("files %x wav%s" % (version, " unity" if at_unity else ""), C.encode_files(ctx, every_format, version, at_unity=at_unity))
            run("files %x flac%s" % (version, " unity" if at_unity else ""), C.encode_files(ctx, flacs, version, at_unity=at_unity))
            run("files %x dcsa%s" % (version, " unity" if at_unity else ""), C.encode_files(ctx, boxes, version, at_unity=at_unity))
            for lname, level in levels() + [("per_file", per_stream(len(mixed)))]:
                if version != 0x9400 and lname.endswith("+clip"):
                    continue
                run("files %x mixed %s%s" % (version, lname, " unity" if at_unity else ""),
                    C.encode_files(ctx, mixed, version, at_unity=at_unity, level=level))
    # one long file among short ones: its walk goes to the host pool
    long_file = WC.wav("s16", 1, 44100, WC.signal("s16", 120000, 0x180))
    for lname, level in (("none", None), ("fit0.5", Level(LEVEL_FIT, ceiling=0.5))):
        run("files host walk %s" % lname, C.encode_files(ctx, [every_format[2], long_file, flacs[0]], level=level))
    loud_wav = wav["fullscale_s16_31250"]
    empty_box = D.dcsa_header(D.format_os(D.FMT_94_T0), 4) + bytes(4)
    nan_wav = dict(WC.float_edge_cases())["fe_f32_nan_1ch"]
    bad_flac = dict((c[0], c[1]) for c in FC.refused_cases())["r23_length_mismatch"]        # (refused by F1 on the device)
    for lname, level in (("none", None), ("gain1", unit), ("fit", fit)):
        run("refuse files loud,plan %s" % lname, C.encode_files(ctx, [loud_wav, wav["err_mulaw"]], at_unity=True, level=level))
        run("refuse files empty box,loud %s" % lname, C.encode_files(ctx, [empty_box, loud_wav], 0x9302, at_unity=True, level=level))
        run("refuse files box,loud %s" % lname, C.encode_files(ctx, [boxes[0], loud_wav], 0x9302, at_unity=True, level=level))
        run("refuse files short %s" % lname, C.encode_files(ctx, mixed, level=level, short=1))
        run("refuse files nan %s" % lname, C.encode_files(ctx, [every_format[2], nan_wav], level=level))
        run("refuse files flac frame %s" % lname, C.encode_files(ctx, [flacs[0], bad_flac], level=level))
        run("files empty %s" % lname, C.encode_files(ctx, [], level=level))
    run("refuse files level+junk", C.encode_files(ctx, [b"junk" * 20, every_format[2]], level=[fit, Level(LEVEL_GAIN, gain=-1.0)]))
    run("refuse files gain1.01", C.encode_files(ctx, mixed, level=[fit, fit, Level(LEVEL_GAIN, gain=1.01)] + [fit] * 5))
    run("refuse files type1", C.encode_files(ctx, mixed, 0x9301, streamFormatType=1))
    run("refuse files tiny", C.encode_files(ctx, [every_format[2], WC.wav("f32", 1, 384000, np.full(3, 0.1))]))
    ctx.close()
    print("# %d calls" % len(calls))
    return 0


if __name__ == "__main__":
    sys.exit(main())
