"""numpy restatement of libnyquist's WAV reader as dcs_wav_parse / dcs_wav_decode define it (WavDecoder.cpp LoadFromBuffer,
Common.cpp ReadFile / ConvertToFloat32, Common.h ScanForChunk and the *_to_float32 macros), with the library's numbered rules
("Encoding files") where libnyquist is undefined or departs from the format, and EncodeFile's downmix."""
import struct

import numpy as np

OK, INVALID_ARG, BAD_STREAM = 0, -1, -6
U8, S16, S24, S32, F32, F64, IMA = range(7)
WIDTH = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4, F64: 8}
GUID_TAIL = bytes([0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])
IMA_STEP = np.array([7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107,
                     118, 130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876,
                     963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871,
                     5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385,
                     24623, 27086, 29794, 32767])
IMA_INDEX = [-1, -1, -1, -1, 2, 4, 6, 8, -1, -1, -1, -1, 2, 4, 6, 8]


def scan(b, code):
    """ScanForChunk: the first 2-byte-aligned match whose 8 bytes lie in the file -> (offset, size); (0, 0) for none"""
    c = code.encode()
    for i in range(0, len(b) - 7, 2):
        if b[i:i + 4] == c:
            return i, struct.unpack_from("<I", b, i + 4)[0]
    return 0, 0


def parse(b):
    """-> (status, dict); the dict has the DcsWavInfo fields that apply"""
    b = bytes(b)
    d = {}
    if len(b) < 64:
        return INVALID_ARG, d
    if b[:4] != b"RIFF":
        return INVALID_ARG, d
    if b[8:12] != b"WAVE" or struct.unpack_from("<I", b, 4)[0] + 8 != len(b):
        return INVALID_ARG, d
    fo, _ = scan(b, "fmt ")
    if fo == 0:
        return INVALID_ARG, d
    if fo + 24 > len(b):
        return BAD_STREAM, d
    size, code, ch, rate, _, ba, bits = struct.unpack_from("<IHHIIHH", b, fo + 4)
    if size < 16:
        return INVALID_ARG, d
    d.update(formatCode=code, channels=ch, rate=rate, blockAlign=ba, bitDepth=bits)
    is_float = code == 3
    if code == 0xFFFE:
        if size < 40:
            return INVALID_ARG, d
        if fo + 48 > len(b):
            return BAD_STREAM, d
        sub = struct.unpack_from("<I", b, fo + 32)[0]
        if sub not in (1, 3) or b[fo + 36:fo + 48] != GUID_TAIL:
            return INVALID_ARG, d
        is_float = sub == 3
        if is_float and bits not in (32, 64):
            return INVALID_ARG, d
    elif code not in (1, 3, 0x11):
        return INVALID_ARG, d
    if code == 0x11:
        if bits != 4:
            return INVALID_ARG, d
        fmt = IMA
    elif bits in (4, 16):
        fmt = S16
    elif bits == 8:
        fmt = U8
    elif bits == 24:
        fmt = S24
    elif bits == 32:
        fmt = F32 if is_float else S32
    elif bits == 64 and is_float:
        fmt = F64
    else:
        return INVALID_ARG, d
    d["sampleFormat"] = fmt
    if ch not in (1, 2):
        return INVALID_ARG, d
    do, ds = scan(b, "data")
    if do == 0:
        return INVALID_ARG, d
    d.update(dataOffset=do + 8, dataSize=ds)
    if do + 8 + ds > len(b):
        return BAD_STREAM, d
    if ba == 0:
        return BAD_STREAM, d
    if fmt != IMA:
        d["nValues"] = (ds // ba) * ch
        if do + 8 + d["nValues"] * WIDTH[fmt] > len(b):
            return BAD_STREAM, d
        return OK, d
    fa, fsz = scan(b, "fact")
    if fsz == 0 or fa + 12 > len(b):
        return BAD_STREAM, d
    total = (struct.unpack_from("<I", b, fa + 8)[0] * ch) & 0xFFFFFFFF
    if ba < 4 * ch or (ba - 4 * ch) % (4 * ch):
        return INVALID_ARG, d
    d["nValues"] = total
    d["nBlocks"] = nb = ds // ba
    if nb * (2 * ba - 8 * ch) > 2 * total:
        return BAD_STREAM, d
    for k in range(nb):
        for c in range(ch):
            h = do + 8 + k * ba + 4 * c
            if b[h + 3] != 0 or b[h + 2] > 88:
                return BAD_STREAM, d
    return OK, d


def ima_decode(b, d):
    """decode_ima_adpcm over the blocks: int16 at libnyquist's offsets, the first nValues kept (the rest zero)"""
    ch, ba, total = d["channels"], d["blockAlign"], d["nValues"]
    out = np.zeros(max(total, 2 * total), np.int16)
    base = d["dataOffset"]
    per = 2 * ba - 8 * ch
    for k in range(d["nBlocks"]):
        blk = b[base + k * ba:base + (k + 1) * ba]
        off = k * per
        for c in range(ch):
            p = struct.unpack_from("<h", blk, 4 * c)[0]
            s = blk[4 * c + 2]
            byte = 4 * ch + 4 * c
            idx = c
            while byte < ba:
                for _ in range(4):
                    for n in (blk[byte] & 15, blk[byte] >> 4):
                        step = int(IMA_STEP[s])
                        diff = step >> 3
                        if n & 4: diff += step
                        if n & 2: diff += step >> 1
                        if n & 1: diff += step >> 2
                        if n & 8: diff = -diff
                        p = ((p + diff + 32768) & 0xFFFF) - 32768          # int16_t p += diff wraps
                        s = min(88, max(0, s + IMA_INDEX[n]))
                        out[off + idx] = p
                        idx += ch
                    byte += 1
                byte += 4 * (ch - 1)
    return out[:total]


def values(b, d):
    """ConvertToFloat32: the file's float32 values (interleaved)"""
    b = bytes(b)
    fmt, n, o = d["sampleFormat"], d["nValues"], d["dataOffset"]
    if fmt == IMA:
        return ima_decode(b, d).astype(np.float32) / np.float32(32767.0)
    raw = b[o:o + n * WIDTH[fmt]]
    if fmt == U8:
        return (np.frombuffer(raw, np.uint8).astype(np.float32) - np.float32(128)) * np.float32(np.float32(1.0) / np.float32(127.0))
    if fmt == S16:
        return np.frombuffer(raw, "<i2").astype(np.float32) / np.float32(32767.0)
    if fmt == S24:
        u = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        x = u[:, 0] | (u[:, 1] << 8) | (u[:, 2] << 16)
        x = np.where(x & 0x800000, x - (1 << 24), x)
        return x.astype(np.float32) / np.float32(8388608.0)
    if fmt == S32:
        return np.frombuffer(raw, "<i4").astype(np.float32) / np.float32(2147483648.0)
    if fmt == F32:
        return np.frombuffer(raw, "<f4").copy()
    with np.errstate(over="ignore"):        # past FLT_MAX the C cast gives +-inf
        return np.frombuffer(raw, "<f8").astype(np.float32)


def downmix(v, channels):
    """EncodeFile's mono signal: (L + R) / 2.0f per pair, a final unpaired value alone"""
    v = np.asarray(v, np.float32)
    if channels != 2:
        return v
    m = len(v) // 2
    with np.errstate(over="ignore", invalid="ignore"):
        out = (v[0:2 * m:2] + v[1:2 * m:2]) / np.float32(2.0)
    return np.concatenate([out, v[2 * m:]]).astype(np.float32)


def decode(b):
    """-> (status, mono float32 at the file's own rate or None, parse dict)"""
    st, d = parse(b)
    if st != OK:
        return st, None, d
    return OK, downmix(values(b, d), d["channels"]), d
