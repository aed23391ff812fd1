"""numpy restatement of the rate-distortion OS93 Type-0 encoder, from PCM to bytes (test infrastructure, not part of the
product).  There is no reference encoder to equal: the algorithm is the project's own, stated in DESIGN.md 10.12, and this
file is its second statement.  It shares the scale table of dcs_tables.h with the kernels (through enc_ref) and nothing else.

After one f32 multiply and one roundf per coefficient everything is integer (int64; the bounds are in DESIGN.md):
  targets  t[k] = clamp(roundf(-K * f[k]), -32768, 32767), k = 0..255, sample j of band b is k = 16 b + j: the spectrum
           NEGATED, because the OS93 transform turns the polarity of what the frame buffer holds; the decoder puts
           sample k into frame-buffer word k + 1 and then moves word 1 into word 0; word 256 (sample 255) is not read by the
           transform, so t[255] = 0 and its value is 0
  items    per frame, band and scale code e = 0..63: the nearest values q (unclamped), the direct options c = 1..15 (q
           clamped to c + 1 bits) with their squared error against the decoder's word R(q, e) at M0, the band's energy (the
           zero option), and what the delta options need of q: q0, q1, q14, q15 and the widths of the inner differences
  proxy    per band, e and lambda the sum over the frames of the least max(D, E_b) + lambda * bits over the zero and direct
           options, 5 bits of band-type code each: picks the header vector and the band count per lambda
  trellis  per frame and lambda at that header vector: stages = the kept bands, states = the band's options
  choice   per stream the least error within the budget over the 56 candidates, else the fewest bits
"""
import math

import numpy as np

import enc_ref as E

F32 = np.float32
DEFAULTS = dict(E.DEFAULTS)

# the mixing multiplier at volume, level and channel volume 0xFF, every frame but a fresh decoder's first: per formatVersion
M0 = {0x9301: 0xFFFE, 0x9302: 0xFEFC}
OS_OF = {0x9301: 0, 0x9302: 1}
K = F32(32768.0)
KL = 56
LADDER = [0, 1] + [(2 + (k & 1)) << (k >> 1) for k in range(KL - 3)] + [1 << 32]
E_MAX = 1 << 40
INF = 1 << 62
QMAX = np.array([32767 // int(s) for s in E.SCALE], np.int64)
NS = 19                         # states: 0 zero (sub-type 0), 1..15 direct, 16 delta, 17 double delta, 18 hold at (0, 0) (sub-type 2)
Z0, DELTA, DDELTA, Z2 = 0, 16, 17, 18
SUB = np.array([0] * 16 + [1, 2, 2], np.int64)
CODE0 = np.array([1] + [0] * 17 + [1], bool)
assert len(LADDER) == KL


def rcp(version):
    return np.array([(1 << 40) // (int(s) * (M0[version] + 1)) for s in E.SCALE], np.int64)


def recon(q, e, version):
    """the decoder's frame-buffer word for sample value q at scale code e (AddOutput on a zero accumulator, at M0)"""
    p = np.asarray(q, np.int64) * E.SCALE[e]
    low = p & 0xFFFF
    sx = low - ((low & 0x8000) << 1)
    w = ((low + sx * M0[version]) >> 16) & 0xFFFF
    return w - ((w & 0x8000) << 1)


def targets(spec):
    """[F, 256] f32 -> [F, 256] integers: the negated spectrum (the decoders' transform turns the polarity back), the last
    one 0 (its word is not read)"""
    t = np.clip(E.round_away(spec.astype(F32) * -K), -32768, 32767)
    t[:, 255] = 0
    return t


def frame_buffer(rec):
    """reconstructed samples [F, 256] (sample 255 zero) -> the decoder's frame-buffer words 0..255"""
    return np.concatenate([rec[:, :1], np.zeros_like(rec[:, :1]), rec[:, 1:255]], axis=1)


def nearest(t, version):
    """[..., N] -> [..., N, 64]: per scale code the sample value whose word is nearest to the target, |q| <= QMAX[e]: the
    estimate (|t| * rcp[e]) >> 24 with -1, 0, +1 and +2 added, smaller magnitude first, replaced on strictly less"""
    r = rcp(version)
    s = np.sign(t)[..., None]
    a = np.abs(t)[..., None]
    e = np.arange(64)
    est = (a * r[e]) >> 24
    best, berr = None, None
    for d in (-1, 0, 1, 2):
        q = np.clip(s * (est + d), -QMAX[e], QMAX[e])
        err = np.abs(t[..., None] - recon(q, e, version))
        if best is None:
            best, berr = q, err
        else:
            take = err < berr
            best, berr = np.where(take, q, best), np.where(take, err, berr)
    return best


def swidth(v):
    """the least w with -2^(w-1) <= v <= 2^(w-1) - 1, elementwise (1 for 0 and -1)"""
    v = np.asarray(v, np.int64)
    m = np.where(v < 0, ~v, v)
    w = np.zeros(v.shape, np.int64)
    for k in range(18):
        w += (m >> k) > 0
    return w + 1


def wrap16(v):
    v = np.asarray(v, np.int64) & 0xFFFF
    return v - ((v & 0x8000) << 1)


def items(t, version):
    """-> dict: Q [F, 16, 16 samples, 64] unclamped; D [F, 16, 64, 16 options] (option 0: the band's energy); q0, q1, q14,
    q15 [F, 16, 64]; L1, L2 [F, 16, 64] the widths of the inner first (j = 1..15) and second (j = 2..15) differences"""
    F = t.shape[0]
    tb = t.reshape(F, 16, 16)
    Q = nearest(tb, version)                                        # [F, 16, 16, 64]
    e = np.arange(64)
    D = np.zeros((F, 16, 64, 16), np.int64)
    D[:, :, :, 0] = (tb ** 2).sum(axis=2)[:, :, None]
    for c in range(1, 16):
        q = np.clip(Q, -(1 << c), (1 << c) - 1)
        D[:, :, :, c] = ((tb[..., None] - recon(q, e, version)) ** 2).sum(axis=2)
    d1 = np.diff(Q, axis=2)
    d2 = np.diff(d1, axis=2)
    return dict(Q=Q, D=D, q0=Q[:, :, 0], q1=Q[:, :, 1], q14=Q[:, :, 14], q15=Q[:, :, 15],
                L1=swidth(d1).max(axis=2), L2=swidth(d2).max(axis=2))


def band_floor(mqe):
    """E_b, in double: min(floor(((K^2 * q) * q) * 16), 2^40), compared before the value leaves double"""
    q = float(F32(mqe))
    v = math.floor(((1073741824.0 * q) * q) * 16.0)
    return E_MAX if v >= float(E_MAX) else int(v)


OPT_BITS = np.array([5] + [5 + 16 * (c + 1) for c in range(1, 16)], np.int64)      # the proxy's: zero and direct options


def proxy(D, Eb):
    """-> J, B [KL, 16, 64]: per lambda, band and scale code the sums over the frames of the least step cost over the zero
    and direct options (a tie to fewer bits, which is the lower option) and of its bits"""
    md = np.maximum(D, Eb)
    J = np.zeros((KL, 16, 64), np.int64)
    B = np.zeros((KL, 16, 64), np.int64)
    for li, lam in enumerate(LADDER):
        cost = md + lam * OPT_BITS
        arg = cost.argmin(axis=3)
        J[li] = np.take_along_axis(cost, arg[..., None], axis=3)[..., 0].sum(axis=0)
        B[li] = OPT_BITS[arg].sum(axis=0)
    return J, B


def headers(J, B, D0tot):
    """per lambda: each band's scale code (least J, then fewer bits, then the lower e) and the band count n in 1..16
    minimising the kept bands' sums plus the cut bands' energies (a tie to the smaller n) -> hv [KL, 16], n [KL]"""
    hv = np.zeros((KL, 16), np.int64)
    nb = np.zeros(KL, np.int64)
    for li in range(KL):
        Jb = np.zeros(16, np.int64)
        for b in range(16):
            best = 0
            for e in range(1, 64):
                if (int(J[li, b, e]), int(B[li, b, e])) < (int(J[li, b, best]), int(B[li, b, best])):
                    best = e
            hv[li, b], Jb[b] = best, J[li, b, best]
        best = None
        for n in range(1, 17):
            tot = int(Jb[:n].sum()) + int(D0tot[n:].sum())
            if best is None or tot < best[0]:
                best = (tot, n)
        nb[li] = best[1]
    return hv, nb


def band_states(it, b, fr, e):
    """of band b, per row (frame fr[r] at scale code e[r]) and state: D [R, NS], outgoing P and Dl [R, NS] (signed 16-bit)"""
    D = it["D"][fr, b, e, :]
    R = D.shape[0]
    q14, q15 = it["q14"][fr, b, e], it["q15"][fr, b, e]
    Ds = np.zeros((R, NS), np.int64)
    P = np.zeros((R, NS), np.int64)
    Dl = np.zeros((R, NS), np.int64)
    Ds[:, Z0] = Ds[:, Z2] = D[:, 0]
    for c in range(1, 16):
        lo, hi = -(1 << c), (1 << c) - 1
        Ds[:, c] = D[:, c]
        P[:, c] = np.clip(q15, lo, hi)
        Dl[:, c] = wrap16(P[:, c] - np.clip(q14, lo, hi))
    for s in (DELTA, DDELTA):
        Ds[:, s] = D[:, 15]
        P[:, s] = q15
        Dl[:, s] = wrap16(q15 - q14)
    return Ds, P, Dl


def step_bits(it, b, fr, e, pP, pDl, first):
    """bits of the step p -> s in band b, per row: [R, NS (p), NS (s)], -1 where there is none.  pP, pDl [R, NS]: the
    predecessors' outgoing state.  first: band 0, whose one predecessor is the start state standing in as DDELTA (sub-type
    2, no reuse flag, (0, 0)) and may be followed by the hold Z2"""
    R = pP.shape[0]
    q0, q1 = it["q0"][fr, b, e][:, None], it["q1"][fr, b, e][:, None]
    L1, L2 = it["L1"][fr, b, e][:, None], it["L2"][fr, b, e][:, None]
    bits = np.full((R, NS, NS), -1, np.int64)
    flag = CODE0.astype(np.int64)[None, :]                          # the reuse bit is read
    for s in range(NS):
        head = flag + np.where(SUB[None, :] == SUB[s], 5, 6)        # [1, NS]
        if s in (Z0, Z2):
            v = np.where(CODE0[None, :] & (SUB[None, :] == SUB[s]), 1, head) + np.zeros((R, 1), np.int64)
            if s == Z2:
                ok = np.zeros(NS, bool)
                ok[Z2] = True
                ok[DDELTA] = first
                v = np.where(ok[None, :], v, -1)
        elif s < 16:
            v = head + 16 * (s + 1) + np.zeros((R, 1), np.int64)
        elif s == DELTA:
            w = np.maximum(np.maximum(swidth(q0 - pP), L1), 2)
            v = np.where(w <= 16, head + 16 * w, -1)
        else:
            w = np.maximum(np.maximum(np.maximum(swidth(q0 - pP - pDl), swidth(q1 - 2 * q0 + pP)), L2), 2)
            v = np.where(w <= 16, head + 16 * w, -1)
        bits[:, :, s] = v
    return bits


def trellis(it, fr, hv, n, lam, Eb, keep_path=False):
    """one trellis per row r: frame fr[r] at header vector hv[r] (scale codes [R, 16]), n[r] bands kept, multiplier lam[r]
    -> (D [R], bits [R], states [R, 16] or None; a band from n[r] on has state -1)"""
    R = len(fr)
    V = np.full((R, NS), INF, np.int64)
    V[:, DDELTA] = 0                                                # the start state
    TD = np.zeros((R, NS), np.int64)
    TB = np.zeros((R, NS), np.int64)
    pP = np.zeros((R, NS), np.int64)
    pDl = np.zeros((R, NS), np.int64)
    surv = np.zeros((R, 16, NS), np.int64)
    for b in range(int(n.max())):
        e = hv[:, b]
        Ds, P, Dl = band_states(it, b, fr, e)
        bits = step_bits(it, b, fr, e, pP, pDl, b == 0)
        ok = (bits >= 0) & (V < INF)[:, :, None]
        cost = np.where(V < INF, V, 0)[:, :, None] + np.maximum(Ds, Eb)[:, None, :] + lam[:, None, None] * bits
        nbits = TB[:, :, None] + bits
        # least cost, then fewer bits in all, then the lower predecessor: a cost is below 2^46 and the bits below 2^13
        key = np.where(ok, (cost << 13) | nbits, np.iinfo(np.int64).max)
        best = key.argmin(axis=1)
        g = lambda a: np.take_along_axis(a, best[:, None, :], axis=1)[:, 0, :]
        live = g(ok)
        nV = np.where(live, g(cost), INF)
        nTD = np.where(live, np.take_along_axis(TD, best, axis=1) + Ds, 0)
        nTB = np.where(live, g(nbits), 0)
        act = (b < n)[:, None]
        V, TD, TB = np.where(act, nV, V), np.where(act, nTD, TD), np.where(act, nTB, TB)
        pP, pDl = np.where(act, P, pP), np.where(act, Dl, pDl)
        surv[:, b, :] = best
    end = np.zeros(R, np.int64)
    rows = np.arange(R)
    for s in range(1, NS):
        better = (V[:, s] < V[rows, end]) | ((V[:, s] == V[rows, end]) & (TB[:, s] < TB[rows, end]))
        end = np.where(better, s, end)
    states = None
    if keep_path:
        states = np.full((R, 16), -1, np.int64)
        s = end.copy()
        for b in range(15, -1, -1):
            act = b < n
            states[:, b] = np.where(act, s, -1)
            s = np.where(act, surv[rows, b, s], s)
    return TD[rows, end], TB[rows, end], states


def analyse(pcm, version=0x9302):
    """what does not depend on the parameters: the targets and the items"""
    x = E.to_float(pcm)
    if len(x) == 0 or (len(x) + 239) // 240 > 65535:
        raise ValueError("empty stream or more than 65 535 frames")
    t = targets(E.analyse(E.frames_of(x)))
    return dict(x=x, t=t, version=version, it=items(t, version), search={})


def search(an, mqe):
    """everything that does not read the budget, under one error floor: per lambda the header vector, the band count and the
    exact trellis's totals -> dict(hv [KL, 16], n [KL], D [KL], bits [KL])"""
    key = float(F32(mqe))
    if key not in an["search"]:
        it = an["it"]
        Eb = band_floor(key)
        D0tot = it["D"][:, :, 0, 0].sum(axis=0)
        J, B = proxy(it["D"], Eb)
        hv, nb = headers(J, B, D0tot)
        F = it["D"].shape[0]
        fr = np.tile(np.arange(F), KL)
        rep = lambda a: np.repeat(a, F, axis=0)
        d, bits, _ = trellis(it, fr, rep(hv), rep(nb), rep(np.array(LADDER, np.int64)), Eb)
        cut = np.array([int(D0tot[int(n):].sum()) for n in nb], np.int64)
        Dc, Bc = d.reshape(KL, F).sum(axis=1) + cut, bits.reshape(KL, F).sum(axis=1)
        an["search"][key] = dict(hv=hv, n=nb, D=Dc, bits=Bc, J=J, B=B)
    return an["search"][key]


def budget_bits(F, rate=None, budget_bytes=None):
    if budget_bytes is None:
        return (int(rate) * F * 240) // 31250
    return (int(budget_bytes) - 18) * 8 if budget_bytes >= 18 else -1


def choose(an, mqe, budget):
    """-> dict(type, sub, ladderIndex, numBands, frameBits, budgetBits, sqErr, fits, hv)"""
    sr = search(an, mqe)
    cands = [(int(sr["D"][li]), int(sr["bits"][li]), li) for li in range(KL)]
    fit = [c for c in cands if c[1] <= budget]
    best = min(fit) if fit else min(cands, key=lambda c: (c[1], c[2]))
    li = best[2]
    return dict(type=0, sub=0, ladderIndex=li, numBands=int(sr["n"][li]), frameBits=best[1], budgetBits=max(budget, 0),
                sqErr=best[0], fits=bool(fit), hv=sr["hv"][li].copy())


def emit(an, ch, mqe):
    """the chosen candidate's stream bytes, its reconstruction [F, 256] and its states [F, numBands]"""
    it, t, ver = an["it"], an["t"], an["version"]
    F = t.shape[0]
    n, hv = ch["numBands"], ch["hv"]
    rows = np.arange(F)
    d, bits, st = trellis(it, rows, np.tile(hv, (F, 1)), np.full(F, n), np.full(F, LADDER[ch["ladderIndex"]], np.int64),
                          band_floor(float(F32(mqe))), True)
    st = st[:, :n]
    rec = np.zeros((F, 256), np.int64)
    cols_v, cols_n = [], []
    pS = np.full(F, DDELTA, np.int64)
    pP, pDl = np.zeros(F, np.int64), np.zeros(F, np.int64)
    for b in range(n):
        e = int(hv[b])
        s = st[:, b]
        q = it["Q"][:, b, :, e]                                     # [F, 16]
        c = np.where((s >= 1) & (s <= 15), s, 15)
        lo, hi = -(1 << c)[:, None], ((1 << c) - 1)[:, None]
        val = np.where(CODE0[s][:, None], 0, np.clip(q, lo, hi))
        rec[:, 16 * b:16 * b + 16] = np.where(CODE0[s][:, None], 0, recon(val, e, ver))
        d1 = np.hstack([val[:, :1] - pP[:, None], np.diff(val, axis=1)])
        d2 = np.hstack([val[:, :1] - (pP + pDl)[:, None], val[:, 1:2] - 2 * val[:, :1] + pP[:, None], np.diff(val, n=2, axis=1)])
        sym = np.where((s == DELTA)[:, None], d1, np.where((s == DDELTA)[:, None], d2, val))
        w = np.where(s == DELTA, np.maximum(swidth(d1).max(axis=1), 2), np.where(s == DDELTA, np.maximum(swidth(d2).max(axis=1), 2), c + 1))
        w = np.where(CODE0[s], 0, w)
        assert (w <= 16).all()
        reuse = CODE0[pS] & CODE0[s] & (SUB[pS] == SUB[s])
        # the reuse bit (read when the predecessor's code was 0)
        cols_v.append(reuse.astype(np.int64)); cols_n.append(CODE0[pS].astype(np.int64))
        same = SUB[pS] == SUB[s]
        code = np.where(CODE0[s], 0, w - 1)
        inc = (SUB[s] == (SUB[pS] + 1) % 3).astype(np.int64)
        cols_v.append(np.where(same, code, (1 << 5) | (inc << 4) | code)); cols_n.append(np.where(reuse, 0, np.where(same, 5, 6)))
        for j in range(16):
            cols_v.append(sym[:, j] & ((1 << w) - 1)); cols_n.append(w)
        outP = np.where(CODE0[s], 0, val[:, 15])
        outDl = np.where(CODE0[s], 0, wrap16(val[:, 15] - val[:, 14]))
        pS, pP, pDl = s, outP, outDl
    lens = np.stack(cols_n, 1)
    body = E.pack_bits(np.stack(cols_v, 1).ravel(), lens.ravel())
    assert np.array_equal(lens.sum(axis=1), bits) and int(lens.sum()) == ch["frameBits"], (int(lens.sum()), ch["frameBits"])
    D0cut = int((t[:, 16 * n:] ** 2).sum())
    assert int(((t - rec) ** 2).sum()) == ch["sqErr"] == int(d.sum()) + D0cut
    hdr = np.full(16, 0xFF, np.int64)
    hdr[:n] = hv[:n]
    return bytes([F >> 8, F & 0xFF]) + hdr.astype(np.uint8).tobytes() + body, rec, st


def encode(an, budget_bytes=None, **params):
    """-> (stream bytes, info dict, reconstruction [F, 256], states [F, numBands])"""
    p = dict(DEFAULTS, **params)
    F = an["t"].shape[0]
    budget = budget_bits(F, p["targetBitRate"], budget_bytes)
    ch = choose(an, p["maximumQuantizationError"], budget)
    s, rec, st = emit(an, ch, p["maximumQuantizationError"])
    assert len(s) == 18 + (ch["frameBits"] + 7) // 8
    return s, ch, rec, st


MAX_FRAME_BITS = 16 * (1 + 6 + 16 * 16)         # every band behind a zero band, changing the sub-type, at 16 bits a value


def bound(n_samples):
    """the longest stream n_samples samples can encode to (0 = not encodable)"""
    nf = (n_samples + 239) // 240
    if nf == 0 or nf > 65535:
        return 0
    return 18 + (nf * MAX_FRAME_BITS + 7) // 8
