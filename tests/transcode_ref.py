"""The transcoding composition on the CPU (test infrastructure): what dcs_transcode_streams writes, restated.

EncodeDCSFile's rule (DCSEncoder.cpp:498-517): a source whose version is the target's, or an OS93 Type-0 source for an OS93
target, is copied; any other one is decoded as the reference's recipe plays it -- InitStandalone + SoftBoot (master volume
0x67), LoadAudioStream(0, stream, 0xFF), nFrames + 1 frames -- and the int16 samples, x / 32768, go to the encoder.  The
decode here is the oracle's C restatement (oracle/dcs_oracle.c; tests/test_oracle_vs_ref.py pins it to the reference), the
encode the numpy restatements (enc_ref.py, enc93_ref.py).  INTEGRATION.md "Transcoding" states the rule and its departures."""
import numpy as np

import dcsexplorer_amd as D
import enc_ref as E
import enc93_ref as R

VERSION = {D.OS93A: 0x9301, D.OS93B: 0x9302, D.OS94: 0x9400, D.OS95: 0x9400}
COPIED, REENCODED = D.TRANSCODE_COPIED, D.TRANSCODE_REENCODED
RECIPE = dict(volume=0x67, level=0xFF)


def frames(stream):
    return (stream[0] << 8) | stream[1]


def action(stream, os_, version, reencode_all=False):
    v = VERSION[os_]
    if not reencode_all and (v == version or (v >> 8 == 0x93 and version >> 8 == 0x93 and not stream[2] & 0x80)):
        return COPIED
    return REENCODED


def decoded(checker, stream, os_, volume=0x67, level=0xFF):
    """the recipe's int16 PCM, flat: nFrames + 1 frames of 240 samples"""
    return checker.decode(os_, volume, [stream], [level], frames(stream) + 1).ravel()


def encode(pcm, version, typ=-1, sub=-1, **params):
    """-> (stream bytes, times the OS93 Keep +15 rule fired); int16 pcm goes in as x / 32768"""
    if version == 0x9400:
        return E.encode(pcm, (typ, sub), **params)[0], 0
    s, _, _, fired = R.encode(pcm, version, typ, **params)
    return s, fired


def transcode(checker, stream, os_, version, typ=-1, sub=-1, reencode_all=False, volume=0x67, level=0xFF, **params):
    """-> (the bytes dcs_transcode_streams writes for one source, its action)"""
    if action(stream, os_, version, reencode_all) == COPIED:
        return bytes(stream), COPIED
    return encode(decoded(checker, stream, os_, volume, level), version, typ, sub, **params)[0], REENCODED
