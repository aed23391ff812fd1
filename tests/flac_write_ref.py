"""A numpy restatement of the FLAC writer (INTEGRATION.md "Writing FLAC"): the choice of each block's subframe and the bit
writer, from the rules stated there and the FLAC format.  Mono, 16 bits, fixed block size 4096, fixed predictors of order
0..4 with partitioned Rice coding (4-bit parameters, partition orders 0..4, never an escape), CONSTANT for a block of one
value, VERBATIM wherever FIXED would not be smaller.

  write(pcm, rate, md5) -> (bytes, info)      one stream; info has the DcsFlacWriteInfo fields
  choose(s)             -> the block's record  kind, order, partition order, parameters, bits behind the subframe header
"""
import hashlib

import numpy as np

BLOCK = 4096
FRAME = 240
CONSTANT, VERBATIM, FIXED = 0, 1, 2
MAX_FRAME = 16 + 1 + 2 * BLOCK + 2          # dcs_flac_write_bound's bytes per block


def write_bound(n_samples):
    return 42 + ((n_samples + BLOCK - 1) // BLOCK) * MAX_FRAME


def utf8(v):
    """the format's UTF-8-style coding of a frame number, general form (up to 36 bits)"""
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >> (5 * n + 1):                 # n bytes hold 7 - n + 6 (n - 1) = 5 n + 1 bits
        n += 1
    out = [((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))]
    for i in range(n - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * i)) & 0x3F))
    return bytes(out)


def _table(poly, bits):
    t = []
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    for b in range(256):
        c = b << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        t.append(c)
    return t


_T8, _T16 = _table(0x07, 8), _table(0x8005, 16)


def crc8(b):
    c = 0
    for x in b:
        c = _T8[c ^ x]
    return c


def crc16_serial(b):
    c = 0
    for x in b:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ x]
    return c


# what byte value b contributes to the CRC-16 when m bytes follow it: _T16 moved on by m zero bytes (a CRC is linear)
_CONTRIB = None


def crc16(b):
    global _CONTRIB
    if len(b) < 64:
        return crc16_serial(b)
    if _CONTRIB is None:
        t16 = np.array(_T16, np.uint16)
        c = np.zeros((MAX_FRAME, 256), np.uint16)
        c[0] = t16
        for m in range(1, MAX_FRAME):
            p = c[m - 1]
            c[m] = (p << 8) ^ t16[p >> 8]
        _CONTRIB = c
    a = np.frombuffer(b, np.uint8)
    return int(np.bitwise_xor.reduce(_CONTRIB[np.arange(a.size - 1, -1, -1), a]))


def residual(s, order):
    """the fixed predictor's residual as plain finite differences; entries below `order` are not residuals"""
    e = np.asarray(s, np.int64)
    for _ in range(order):
        e = np.concatenate(([0], np.diff(e)))
    return e


def choose(s, constrain=True):
    """constrain=False: without the rule that a partition is longer than the warm-up (to see where the rule binds; never written)"""
    s = np.asarray(s, np.int64)
    n = s.size
    assert n % 16 == 0 and 16 <= n <= BLOCK
    if (s == s[0]).all():
        return dict(kind=CONSTANT, order=0, p=0, k=[], bits=16)
    sums = [int(np.abs(residual(s, o)[4:]).sum()) for o in range(5)]
    order = int(np.argmin(sums))                                    # (ties: the lowest order)
    e = residual(s, order)
    u = np.where(e >= 0, 2 * e, -2 * e - 1)
    u[:order] = 0
    # residuals per finest partition: its samples from `order` on (none where a short block's partition lies in the warm-up)
    count = np.clip((np.arange(16) + 1) * (n // 16) - order, 0, n // 16)
    parts = u.reshape(16, n // 16)
    B = np.stack([(parts >> k).sum(axis=1) + (k + 1) * count for k in range(15)], axis=1)       # [16][15]
    best = None
    for p in range(4, -1, -1):
        ks = B.argmin(axis=1)                                       # (ties: the lowest parameter)
        total = int(B.min(axis=1).sum()) + 4 * (1 << p)
        # a candidate only where a partition is longer than the warm-up, as the format asks; p = 0 always is (n >= 16 > 4)
        if ((n >> p) > order or not constrain) and (best is None or total <= best[0]): # (ties: the lowest partition order)
            best = (total, p, [int(k) for k in ks])
        B = B[0::2] + B[1::2]
    total, p, ks = best
    if 6 + total >= 16 * (n - order):
        return dict(kind=VERBATIM, order=0, p=0, k=[], bits=16 * n)
    return dict(kind=FIXED, order=order, p=p, k=ks, bits=16 * order + 6 + total)


def _pack(values, lengths):
    """fields of `lengths` bits (0..32) holding `values`, first field first, most significant bit first -> (bytes, bits)"""
    values, lengths = np.asarray(values, np.int64), np.asarray(lengths, np.int64)
    end = np.cumsum(lengths)
    total = int(end[-1])
    bits = np.zeros((total + 7) // 8 * 8, np.uint8)
    start = end - lengths
    for b in range(int(lengths[values != 0].max()) if (values != 0).any() else 0):
        m = (lengths > b) & (((values >> np.maximum(lengths - 1 - b, 0)) & 1) != 0)
        bits[start[m] + b] = 1
    return np.packbits(bits).tobytes(), total


_SUBFRAMES = {}


def subframe(s):
    """-> (record, the subframe's bytes, zero padded to a byte); a block's subframe does not depend on where the block lies"""
    s = np.asarray(s, np.int64)
    key = s.astype("<i2").tobytes()
    if key in _SUBFRAMES:
        return _SUBFRAMES[key]
    c = choose(s)
    n = s.size
    if c["kind"] == CONSTANT:
        body = bytes([0x00]) + int(s[0] & 0xFFFF).to_bytes(2, "big")
    elif c["kind"] == VERBATIM:
        body = bytes([0x02]) + s.astype(">i2").tobytes()
    else:
        o, p = c["order"], c["p"]
        e = residual(s, o)[o:]
        u = np.where(e >= 0, 2 * e, -2 * e - 1)
        size = n >> p
        part = (np.arange(o, n) // size)
        k = np.asarray(c["k"], np.int64)[part]
        q = u >> k
        first = np.concatenate(([True], part[1:] != part[:-1]))
        # per residual: [the partition's parameter, 4 bits, in front of its first residual], q zeros, a one and the k low bits
        vals = np.stack([k, np.zeros_like(q), (1 << k) | (u & ((1 << k) - 1))], axis=1)
        lens = np.stack([np.where(first, 4, 0), q, k + 1], axis=1)
        # (q may exceed 32: a field of zeros of any length is fine, _pack never looks at its value)
        head_v = [0x10 | (o << 1)] + [int(x) & 0xFFFF for x in s[:o]] + [0, p]
        head_l = [8] + [16] * o + [2, 4]
        body, nbits = _pack(np.concatenate((head_v, vals.ravel())), np.concatenate((head_l, lens.ravel())))
        assert nbits == 8 + c["bits"], (nbits, c)
    _SUBFRAMES[key] = (c, body)
    if len(_SUBFRAMES) > 4096:
        _SUBFRAMES.pop(next(iter(_SUBFRAMES)))
    return c, body


def frame_header(number, n, rate):
    if n == BLOCK:
        code, extra = 0xC, b""
    elif n <= 256:
        code, extra = 0x6, bytes([n - 1])
    else:
        code, extra = 0x7, (n - 1).to_bytes(2, "big")
    h = bytes([0xFF, 0xF8, (code << 4) | 0xD, 0x08]) + utf8(number) + extra + rate.to_bytes(2, "big")
    return h + bytes([crc8(h)])


def frame(s, number, rate):
    c, body = subframe(s)
    f = frame_header(number, len(s), rate) + body
    return c, f + crc16(f).to_bytes(2, "big")


def write(pcm, rate=31250, md5=True):
    s = np.asarray(pcm).astype(np.int64).ravel()
    assert s.size >= FRAME and s.size % FRAME == 0 and 1 <= rate <= 65535 and s.size < 1 << 36
    frames, kinds = [], [0, 0, 0]
    for b in range(0, s.size, BLOCK):
        c, f = frame(s[b:b + BLOCK], b // BLOCK, rate)
        kinds[c["kind"]] += 1
        frames.append(f)
    lo, hi = min(map(len, frames)), max(map(len, frames))
    digest = hashlib.md5(s.astype("<i2").tobytes()).digest() if md5 else bytes(16)
    v = (rate << 44) | (0 << 41) | (15 << 36) | s.size
    info = (BLOCK.to_bytes(2, "big") * 2 + lo.to_bytes(3, "big") + hi.to_bytes(3, "big") + v.to_bytes(8, "big") + digest)
    out = b"fLaC" + bytes([0x80, 0, 0, 34]) + info + b"".join(frames)
    return out, dict(nSamples=s.size, nBytes=len(out), nBlocks=len(frames), nConstant=kinds[CONSTANT], nVerbatim=kinds[VERBATIM],
                     nFixed=kinds[FIXED], minFrame=lo, maxFrame=hi)
