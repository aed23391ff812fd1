"""numpy restatement of the OS93a Type-1 (pair-table) encoder, from PCM to bytes (test infrastructure, not part of the
product).  There is no reference encoder for this layout: the algorithm is the project's own, stated in DESIGN.md 10.10,
and this file is its second statement.  It shares the constant tables of dcs_tables.h with the kernels and nothing else.

After one f32 multiply and one roundf per coefficient everything is integer (Python ints / int64):
  targets   t[i] = clamp(roundf(K * f[i - 1]), -32768, 32767) for frame-buffer word i >= 2, t[0] from f[0], t[1] = 0; K = 32768,
            f = the analysis transform's frame (enc_ref.analyse)
  search    D(b, w, s) = sum over the band's pairs of min_j |t - R(s, w, j)|^2, R the decoder's reconstruction at M0
  walk      per frame, codebook pp and lambda of the ladder: bands in order, minimising max(D, E_b) + lambda * bits,
            E_b = min(floor(2^30 q^2 * 2 inputs), 2^40)
  choice    per stream: the least sum of D among the (pp, lambda) within the byte budget, else the fewest bits
"""
import math

import numpy as np

import enc_ref as E
import enc93_ref as E93

F32 = np.float32
DEFAULTS = dict(E.DEFAULTS)

M0 = 0xFFFE                     # OS93a's mixing multiplier at mixing level 0xFF, the level transcoding and the sweep decode at
K = F32(32768.0)                # spec 1.0 = frame-buffer 32768 at M0
NS = 4                          # scale codes searched per (band, width)
S_MIN, S_MAX = 4, 0x39
KL = 64                         # the ladder's entries
LADDER = [0] + [(2 + (k & 1)) << (k >> 1) for k in range(1, KL - 1)] + [1 << 40]
WMAX = [5, 7, 8, 9]
INPUTS = np.array(E._ints(E._D["kInputsPerBand93a"]))
FIRST = np.concatenate([[0], np.cumsum(INPUTS)[:-1]])           # in pairs
PRV0 = 0x1A


def _sx16(v):
    v = np.asarray(v, np.int64) & 0xFFFF
    return v - ((v & 0x8000) << 1)


PAIR = _sx16(E._ints(E._D["kPair93a"]))


def pairs_of(w):
    """the 2^w points of width w: [2^w, 2]"""
    return PAIR[(2 << w):(2 << w) + (2 << w)].reshape(-1, 2)


def _sfs(s):
    sf = 0x8000
    for _ in range(s & 3):
        sf = (sf * 0x9838) >> 15
    sf = (sf << (s >> 2)) & 0xFFFFFFFF
    sf = (((sf >> 16) * M0) & 0xFFFFFFFF) >> 15
    return int(_sx16(sf))


SFS = np.array([_sfs(s) for s in range(64)], np.int64)
PMAX = np.array([0] + [int(np.abs(pairs_of(w)).max()) for w in range(1, 10)], np.int64)
REACH = (PMAX[:, None] * SFS[None, :]) >> 15                     # [w][s]


def recon(p):
    """MultiplyRoundAdd on a zero accumulator: p = pair * sfs -> the frame-buffer word, as a signed integer"""
    p = np.asarray(p, np.int64)
    mr = ((p << 1) + 0x8000) & 0xFFFFFFFF
    mr = np.where((p & 0x7FFF) == 0x4000, mr & ~np.int64(0x10000), mr)
    mr = mr - ((mr & 0x80000000) << 1)
    return mr >> 16


def _books():
    bb = E._ints(E._D["kBandBits93a"])
    plen, pcode = np.zeros((4, 10), np.int64), np.zeros((4, 10), np.int64)
    term = []
    for pp in range(4):
        for i in range(16):
            e = bb[pp * 16 + i]
            n, w = e >> 8, e & 0xFF
            if w == 0xFF:
                term.append((i >> (4 - n), n))
            elif plen[pp, w] == 0:
                plen[pp, w], pcode[pp, w] = n, i >> (4 - n)
    sc = E._ints(E._D["kScaleCb93a"])
    dlen, dcode = np.zeros(54, np.int64), np.zeros(54, np.int64)
    for i in range(16):
        e = sc[i]
        n, v = (e >> 8) & 0xF, e & 0xFF
        if v != 0xFF:
            if dlen[v] == 0:
                dlen[v], dcode[v] = n, i >> (4 - n)
            continue
        for j in range(16):
            e2 = sc[((e >> 12) << 4) + j]
            n2, v2 = (e2 >> 8) & 0xF, e2 & 0xFF
            if dlen[v2] == 0:
                dlen[v2], dcode[v2] = n2, ((i << 4) | j) >> (8 - n2)
    return plen, pcode, term, dlen, dcode


PFX_LEN, PFX_CODE, TERM, DL_LEN, DL_CODE = _books()
assert all(t == (2, 4) for t in TERM) and (DL_LEN > 0).all()
assert all((PFX_LEN[pp, :WMAX[pp] + 1] > 0).all() and (PFX_LEN[pp, WMAX[pp] + 1:] == 0).all() for pp in range(4))


def delta_value(prv, w, s):
    """the codebook value that takes the carried `prv` to scale code s at width w, or -1 where there is none
    (scaleCode = prv + value - 1 + 2w, minus 0x36 above 0x39; value 0..0x35)"""
    v = s - (prv + 2 * w - 1)
    v = np.where(v < 0, v + 54, v)
    return np.where((v >= 0) & (v <= 53), v, -1)


def window_start(peak, w):
    """S(b, w) = NS consecutive codes from here: it ends at the first code whose largest point reaches the band's peak"""
    hi = np.minimum(S_MAX, S_MIN + (REACH[w][None, S_MIN:S_MAX + 1] < np.asarray(peak)[:, None]).sum(axis=1))
    return np.maximum(S_MIN, hi - (NS - 1))


def targets(spec):
    """[F, 256] f32 (the reference's frame.f) -> [F, 254] integers, one per frame-buffer word this decoder writes.  The
    OS93 Type-0 decoder puts f[k] into word k + 1 and then moves word 1 into word 0, so at M0 its frame buffer is
    word 0 = f[0], word 1 = 0, word i = f[i - 1]: these are the targets."""
    v = np.clip(E.round_away(spec.astype(F32) * K), -32768, 32767)
    return np.concatenate([v[:, :1], np.zeros_like(v[:, :1]), v[:, 1:253]], axis=1)


def search(t):
    """-> D0 [F, 18], S0 [F, 18, 10] (window starts), D [F, 18, 10, NS]"""
    F = t.shape[0]
    D0 = np.zeros((F, 18), np.int64)
    S0 = np.zeros((F, 18, 10), np.int64)
    D = np.zeros((F, 18, 10, NS), np.int64)
    for b in range(18):
        tb = t[:, 2 * FIRST[b]:2 * (FIRST[b] + INPUTS[b])].reshape(F, -1, 2)
        D0[:, b] = (tb * tb).sum(axis=(1, 2))
        peak = np.abs(tb).max(axis=(1, 2))
        for w in range(1, 10):
            S0[:, b, w] = window_start(peak, w)
            P = pairs_of(w)
            for k in range(NS):
                R = recon(P[None, :, :] * SFS[S0[:, b, w] + k][:, None, None])          # [F, 2^w, 2]
                d = ((tb[:, :, None, :] - R[:, None, :, :]) ** 2).sum(axis=3)           # [F, n, 2^w]
                D[:, b, w, k] = d.min(axis=2).sum(axis=1)
    return D0, S0, D


E_MAX = 1 << 40                 # E_b saturates here: every D is below 2^38, so from 2^38 on a band's options differ in bits alone


def band_floor(mqe):
    """E_b, in double: min(floor(((K^2 * q) * q) * (2 * inputs)), 2^40), compared before the value leaves double"""
    q = float(F32(mqe))
    e = [math.floor(((1073741824.0 * q) * q) * float(2 * n)) for n in INPUTS]
    return np.array([E_MAX if v >= float(E_MAX) else int(v) for v in e], dtype=object)


def walk(D0, S0, D, mqe):
    """every (frame, pp, lambda) at once -> dict of [F, 4*KL] arrays: L, bitsThrough, sumD, and the choices [F, 4*KL, 18]
    w and s.  Costs stay in int64 (object arrays are avoided): E_b is at most 2^40, D below 2^38, and the ladder's top times
    the most bits a band takes is 2^40 * 264, so a cost is below 2^50."""
    F = D0.shape[0]
    C = 4 * KL
    lam = np.array([LADDER[c % KL] for c in range(C)], np.int64)[None, :]
    pp = np.arange(C) // KL
    Eb = band_floor(mqe)
    prv = np.full((F, C), PRV0, np.int64)
    bits = np.zeros((F, C), np.int64)
    through = np.zeros((F, C), np.int64)
    sumD = np.zeros((F, C), np.int64)
    L = np.full((F, C), -1, np.int64)
    cw, cs = np.zeros((F, C, 18), np.int64), np.zeros((F, C, 18), np.int64)
    for b in range(18):
        n, eb = int(INPUTS[b]), int(Eb[b])
        bb = np.broadcast_to(PFX_LEN[pp, 0][None, :], (F, C)).copy()
        bd = np.broadcast_to(D0[:, b][:, None], (F, C)).copy()
        bc = np.maximum(bd, eb) + lam * bb
        bw, bs = np.zeros((F, C), np.int64), np.zeros((F, C), np.int64)
        for w in range(1, 10):
            ok_w = (np.array(WMAX)[pp] >= w)[None, :]
            for k in range(NS):
                s = S0[:, b, w][:, None] + k
                v = delta_value(prv, w, s)
                nb = PFX_LEN[pp, w][None, :] + DL_LEN[np.maximum(v, 0)] + n * w
                d = np.broadcast_to(D[:, b, w, k][:, None], (F, C))
                cost = np.maximum(d, eb) + lam * nb
                take = ok_w & (v >= 0) & ((cost < bc) | ((cost == bc) & (nb < bb)))
                bc, bb, bd = np.where(take, cost, bc), np.where(take, nb, bb), np.where(take, d, bd)
                bw, bs = np.where(take, w, bw), np.where(take, s + 0 * bw, bs)
        bits = bits + bb
        sumD = sumD + bd
        coded = bw > 0
        prv = np.where(coded, bs - 2 * bw, prv)
        L = np.where(coded, b, L)
        through = np.where(coded, bits, through)
        cw[:, :, b], cs[:, :, b] = bw, bs
    return dict(L=L, through=through, sumD=sumD, w=cw, s=cs)


def budget_bits(rate, F):
    return (int(rate) * F * 240) // 31250


def choose(wk, rate):
    """-> dict(selector, ladderIndex, numBands, frameBits, budgetBits, sqErr, fits)"""
    F = wk["L"].shape[0]
    budget = budget_bits(rate, F)
    cands = []
    for c in range(4 * KL):
        L = wk["L"][:, c]
        nb = max(1, 1 + int(L.max()))
        fb = int(wk["through"][:, c].sum()) + 4 * int((L + 1 < nb).sum())
        cands.append((int(wk["sumD"][:, c].sum()), fb, c, nb))
    fit = [x for x in cands if x[1] <= budget]
    best = min(fit, key=lambda x: (x[0], x[1], x[2])) if fit else min(cands, key=lambda x: (x[1], x[2]))
    return dict(selector=best[2] // KL, ladderIndex=best[2] % KL, numBands=best[3], frameBits=best[1], budgetBits=budget,
                sqErr=best[0], fits=bool(fit))


def emit(t, wk, ch):
    """the chosen candidate's stream bytes and its reconstruction [F, 254]"""
    F = t.shape[0]
    c = ch["selector"] * KL + ch["ladderIndex"]
    pp, nb = ch["selector"], ch["numBands"]
    vals, lens = [], []
    rec = np.zeros((F, 254), np.int64)
    for f in range(F):
        prv, last = PRV0, int(wk["L"][f, c])
        for b in range(last + 1):
            w, s = int(wk["w"][f, c, b]), int(wk["s"][f, c, b])
            vals.append(int(PFX_CODE[pp, w])); lens.append(int(PFX_LEN[pp, w]))
            if w == 0:
                continue
            v = int(delta_value(np.int64(prv), w, np.int64(s)))
            assert v >= 0
            vals.append(int(DL_CODE[v])); lens.append(int(DL_LEN[v]))
            prv = s - 2 * w
            lo, n = 2 * FIRST[b], INPUTS[b]
            tb = t[f, lo:lo + 2 * n].reshape(n, 2)
            R = recon(pairs_of(w) * SFS[s])
            j = ((tb[:, None, :] - R[None, :, :]) ** 2).sum(axis=2).argmin(axis=1)         # (the lowest index of a tie)
            rec[f, lo:lo + 2 * n] = R[j].ravel()
            vals.extend(int(x) for x in j); lens.extend([w] * n)
        if last + 1 < nb:
            vals.append(TERM[pp][0]); lens.append(TERM[pp][1])
    body = E.pack_bits(np.array(vals, np.int64), np.array(lens, np.int64))
    assert sum(lens) == ch["frameBits"]
    return bytes([F >> 8, F & 0xFF, 0x80 | (pp << 5) | nb]) + body, rec


def analyse(pcm):
    """what does not depend on the parameters: the targets and the search"""
    x = E.to_float(pcm)
    if len(x) == 0 or (len(x) + 239) // 240 > 65535:
        raise ValueError("empty stream or more than 65 535 frames")
    t = targets(E.analyse(E.frames_of(x)))
    return dict(x=x, t=t, search=search(t), walks={})


def encode_type1(an, **params):
    """-> (stream bytes, info93a dict, reconstruction [F, 254])"""
    p = dict(DEFAULTS, **params)
    key = float(F32(p["maximumQuantizationError"]))
    if key not in an["walks"]:
        an["walks"][key] = walk(*an["search"], key)
    wk = an["walks"][key]
    ch = choose(wk, p["targetBitRate"])
    s, rec = emit(an["t"], wk, ch)
    return s, ch, rec


def encode(an, typ=1, **params):
    """typ 1, 0 or -1 (both, the first strictly smallest, Type 0 first) -> (stream bytes, type written, numBands /
    bandsToKeep, info93a dict or None where Type 1 was not built)"""
    p = dict(DEFAULTS, **params)
    t0 = E93.encode(an["x"], 0x9301, 0, **p) if typ != 1 else None
    t1 = encode_type1(an, **p) if typ != 0 else None
    if t1 is None or (t0 is not None and len(t0[0]) <= len(t1[0])):
        return t0[0], 0, t0[2], (t1[1] if t1 else None)
    return t1[0], 1, t1[1]["numBands"], t1[1]


MAX_FRAME_BITS = int(sum(4 + 8 + 9 * n for n in INPUTS))        # every band at width 9 with the longest prefix and delta


def bound(n_samples):
    """the longest stream n_samples samples can encode to through dcs_encode93a_streams, either type (0 = not encodable)"""
    nf = (n_samples + 239) // 240
    if nf == 0 or nf > 65535:
        return 0
    return max(E93.bound(n_samples), 3 + (nf * MAX_FRAME_BITS + 7) // 8)
