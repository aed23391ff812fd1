"""The FLAC writer's restatement for streams of any length (INTEGRATION.md "Writing FLAC", rules 9 to 11): the general
choice of a block's subframe, for a block of 1 .. 4096 samples, over tests/flac_write_ref.py's header, packing and CRC
functions.  On blocks that are multiples of 16 samples the choice is flac_write_ref.choose's, and on streams of whole
frames the bytes are flac_write_ref.write's (tests/test_flac_write_any_host.py holds both to that).

  write(pcm, rate, md5) -> (bytes, info)      one stream of any length >= 1; info has the DcsFlacWriteInfo fields
  choose(s)             -> the block's record  kind, order, partition order, parameters, bits behind the subframe header,
                                               and P, the finest partition order the block's length allows
"""
import hashlib

import numpy as np

import flac_write_ref as R

BLOCK, CONSTANT, VERBATIM, FIXED = R.BLOCK, R.CONSTANT, R.VERBATIM, R.FIXED


def finest(n):
    """P = min(4, the number of trailing zero bits of n)"""
    return min(4, (n & -n).bit_length() - 1)


def choose(s, constrain=True):
    """constrain=False: without the rule that a partition is longer than the warm-up (to see where the rule binds; never written)"""
    s = np.asarray(s, np.int64)
    n = s.size
    assert 1 <= n <= BLOCK
    P = finest(n)
    if (s == s[0]).all():                                           # (a block of 1 sample always)
        return dict(kind=CONSTANT, order=0, p=0, k=[], bits=16, P=P)
    sums = [int(np.abs(R.residual(s, o)[4:]).sum()) for o in range(5)]
    order = int(np.argmin(sums))                                    # (ties: the lowest order; n <= 4: every sum is empty, order 0)
    assert order < n
    e = R.residual(s, order)
    u = np.where(e >= 0, 2 * e, -2 * e - 1)
    u[:order] = 0
    size = n >> P
    # residuals per finest partition: its samples from `order` on (none where a partition lies in the warm-up)
    count = np.clip((np.arange(1 << P) + 1) * size - order, 0, size)
    parts = u.reshape(1 << P, size)
    B = np.stack([(parts >> k).sum(axis=1) + (k + 1) * count for k in range(15)], axis=1)       # [2^P][15]
    best = None
    for p in range(P, -1, -1):
        ks = B.argmin(axis=1)                                       # (ties: the lowest parameter)
        total = int(B.min(axis=1).sum()) + 4 * (1 << p)
        # a candidate only where a partition is longer than the warm-up, as the format asks; p = 0 always is (order < n)
        if ((n >> p) > order or not constrain) and (best is None or total <= best[0]):      # (ties: the lowest partition order)
            best = (total, p, [int(k) for k in ks])
        B = B[0::2] + B[1::2]
    total, p, ks = best
    if 6 + total >= 16 * (n - order):
        return dict(kind=VERBATIM, order=0, p=0, k=[], bits=16 * n, P=P)
    return dict(kind=FIXED, order=order, p=p, k=ks, bits=16 * order + 6 + total, P=P)


_SUBFRAMES = {}


def subframe(s):
    """-> (record, the subframe's bytes, zero padded to a byte); a block's subframe does not depend on where the block lies"""
    s = np.asarray(s, np.int64)
    key = s.astype("<i2").tobytes()
    if key not in _SUBFRAMES:
        if len(_SUBFRAMES) >= 8192:
            _SUBFRAMES.pop(next(iter(_SUBFRAMES)))
        _SUBFRAMES[key] = _subframe(s)
    return _SUBFRAMES[key]


def _subframe(s):
    c = choose(s)
    n = s.size
    if c["kind"] == CONSTANT:
        return c, bytes([0x00]) + int(s[0] & 0xFFFF).to_bytes(2, "big")
    if c["kind"] == VERBATIM:
        return c, bytes([0x02]) + s.astype(">i2").tobytes()
    o, p = c["order"], c["p"]
    e = R.residual(s, o)[o:]
    u = np.where(e >= 0, 2 * e, -2 * e - 1)
    part = np.arange(o, n) // (n >> p)
    k = np.asarray(c["k"], np.int64)[part]
    q = u >> k
    first = np.concatenate(([True], part[1:] != part[:-1]))
    # per residual: [the partition's parameter, 4 bits, in front of its first residual], q zeros, a one and the k low bits
    vals = np.stack([k, np.zeros_like(q), (1 << k) | (u & ((1 << k) - 1))], axis=1)
    lens = np.stack([np.where(first, 4, 0), q, k + 1], axis=1)
    head_v = [0x10 | (o << 1)] + [int(x) & 0xFFFF for x in s[:o]] + [0, p]
    head_l = [8] + [16] * o + [2, 4]
    body, nbits = R._pack(np.concatenate((head_v, vals.ravel())), np.concatenate((head_l, lens.ravel())))
    assert nbits == 8 + c["bits"], (nbits, c)
    return c, body


def frame(s, number, rate):
    c, body = subframe(s)
    f = R.frame_header(number, len(s), rate) + body
    return c, f + R.crc16(f).to_bytes(2, "big")


def records(pcm):
    """the records of a stream's blocks, each with its length n"""
    s = np.asarray(pcm).astype(np.int64).ravel()
    return [dict(choose(s[b:b + BLOCK]), n=min(BLOCK, s.size - b)) for b in range(0, s.size, BLOCK)]


def write(pcm, rate, md5=True):
    s = np.asarray(pcm).astype(np.int64).ravel()
    assert 1 <= s.size < 1 << 36 and 1 <= rate <= 65535
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
