"""numpy restatement of the rate-distortion 1994+ encoder, from PCM to bytes (test infrastructure, not part of the product).
There is no reference encoder to equal: the algorithm is the project's own, stated in DESIGN.md 10.11, and this file is
its second statement.  It shares the constant tables of dcs_tables.h with the kernels (through enc_ref) and nothing else.

After one f32 multiply and one roundf per coefficient everything is integer (int64; the bound on a cost is in DESIGN.md):
  targets  t[k] = clamp(roundf(K * f[k]), -32768, 32767), k = 0..254, f the analysis transform's frame; the decoder puts
           sample k into frame-buffer word k + 1 and then moves word 1 into word 0
  items    per frame, band, width w = 1..15 and scale code e = 0..63: the nearest quantisation clamped to the width, its
           squared error against the decoder's word R(q, e) at M0, and its exact sample bits
  trellis  per layout, band, header scale code h of the band's window and lambda of the ladder: states = the previous
           frame's band-type code, step cost max(D, E_b) + lambda * (hdrLen + bits)
  choice   per (layout, lambda) the best h of each band and the best band count; per stream the least error within the
           budget, else the fewest bits
"""
import math

import numpy as np

import enc_ref as E

F32 = np.float32
DEFAULTS = dict(E.DEFAULTS)

M0 = 0xFEFC                     # the 1994+ mixing multiplier at volume, level and channel volume 0xFF, every frame but the first
K = F32(32768.0)                # spec 1.0 = frame-buffer 32768, but for the factor (M0 + 1) / 65536 the search sees through R
KL = 56                         # the ladder's entries
LADDER = [0, 1] + [(2 + (k & 1)) << (k >> 1) for k in range(KL - 3)] + [1 << 32]
NH = 14                         # header scale codes searched per band ...
H_STEP = 3                      # ... this far apart, downwards from ...
H_BASE = (2, 21)                # ... this far below the band's top code (Type 0, Type 1)
LAYOUTS = [(0, 0), (1, 0), (1, 3)]      # searched; (0, 3) is (0, 0) with two header bits set
E_MAX = 1 << 40
INF = 1 << 62
COUNT, FIRST = E.BAND_COUNT, E.BAND_FIRST
QMAX = np.array([32767 // int(s) for s in E.SCALE], np.int64)          # |q * SCALE[e]| stays in 16 bits signed
RCP = np.array([(1 << 40) // (int(s) * (M0 + 1)) for s in E.SCALE], np.int64)
HL = E.HDR_LEN
assert len(LADDER) == KL and all(a < b for a, b in zip(LADDER, LADDER[1:]))


def recon(q, e):
    """the decoder's frame-buffer word for sample value q at scale code e (mixAdd on a zero accumulator, at M0)"""
    p = np.asarray(q, np.int64) * E.SCALE[e]
    low = p & 0xFFFF
    sx = low - ((low & 0x8000) << 1)
    w = ((low + sx * M0) >> 16) & 0xFFFF
    return w - ((w & 0x8000) << 1)


def targets(spec):
    """[F, 256] f32 (the reference's frame.f) -> [F, 255] integers"""
    return np.clip(E.round_away(spec.astype(F32) * K), -32768, 32767)[:, :255]


def frame_buffer(rec):
    """reconstructed samples [F, 255] -> the decoder's frame buffer words 0..255"""
    return np.concatenate([rec[:, :1], np.zeros_like(rec[:, :1]), rec[:, 1:]], axis=1)


def nearest(t):
    """[F, 255] -> [F, 255, 64]: per scale code the sample value whose word is nearest to the target, |q| <= QMAX[e].  The
    estimate (|t| * RCP[e]) >> 24 with -1, 0, +1 and +2 added is tried, smaller magnitude first, replacing on strictly less
    (the word is floor(q * scale * (M0 + 1) / 65536) in magnitude, so the nearest q lies in [est - 1, est + 2])."""
    s = np.sign(t)[:, :, None]
    a = np.abs(t)[:, :, None]
    e = np.arange(64)[None, None, :]
    est = (a * RCP[e]) >> 24
    best, berr = None, None
    for d in (-1, 0, 1, 2):
        q = np.clip(s * (est + d), -QMAX[e], QMAX[e])
        err = np.abs(t[:, :, None] - recon(q, e))
        if best is None:
            best, berr = q, err
        else:
            take = err < berr
            best, berr = np.where(take, q, best), np.where(take, err, berr)
    return best


def items(t):
    """-> D [F, 16 bands, 16 widths, 64 codes] (width 0: the band's energy), B likewise (sample bits), Q0 = nearest(t)"""
    F = t.shape[0]
    Q0 = nearest(t)
    D = np.zeros((F, 16, 16, 64), np.int64)
    B = np.zeros((F, 16, 16, 64), np.int64)
    e = np.arange(64)[None, None, :]
    for b in range(16):
        D[:, b, 0, :] = (t[:, FIRST[b]:FIRST[b] + COUNT[b]] ** 2).sum(axis=1)[:, None]
    for w in range(1, 16):
        q = np.clip(Q0, -(1 << (w - 1)), (1 << (w - 1)) - 1)
        err = (t[:, :, None] - recon(q, e)) ** 2
        for b in range(16):
            s0, n = FIRST[b], COUNT[b]
            D[:, b, w, :] = err[:, s0:s0 + n].sum(axis=1)
            if w > 6:
                B[:, b, w, :] = w * n
                continue
            qb = q[:, s0:s0 + n]
            lens = E.SMP_LEN[w][qb + (1 << (w - 1))]
            z = qb == 0
            run = np.zeros_like(qb)
            for j in range(n):
                run[:, j] = np.where(z[:, j], (run[:, j - 1] + 1) if j else 1, 0)
            nxt = np.concatenate([z[:, 1:], np.zeros_like(z[:, :1])], axis=1)
            lens = np.where(z & (run % 2 == 1) & nxt, E.DZ_LEN[w], np.where(z & (run % 2 == 0), 0, lens))
            B[:, b, w, :] = lens.sum(axis=1)
    return D, B, Q0


def band_floor(mqe):
    """E_b, in double: min(floor(((K^2 * q) * q) * count_b), 2^40), compared before the value leaves double"""
    q = float(F32(mqe))
    e = [math.floor(((1073741824.0 * q) * q) * float(n)) for n in COUNT]
    return np.array([E_MAX if v >= float(E_MAX) else int(v) for v in e], np.int64)


def window(t, typ):
    """[16, NH]: the header scale codes searched per band, from the band's peak over the stream"""
    out = np.zeros((16, NH), np.int64)
    for b in range(16):
        peak = int(np.abs(t[:, FIRST[b]:FIRST[b] + COUNT[b]]).max())
        top = int(np.count_nonzero(E.SCALE < max(peak, 1)))
        out[b] = np.clip(top - H_BASE[typ] - H_STEP * np.arange(NH), 0, 63)
    return out


def pre_map(typ, sub, b):
    return E.PREADJ[0 if sub == 0 else 3] if (typ == 1 and b < 3) else np.zeros(16, np.int64)


def options(typ, b, h, pre):
    """codes 0..15 at header code h and pre-adjust `pre` -> (width, scale code, allowed)"""
    w, sc, _ = E.interpret(typ, b, np.arange(16), h, pre)
    ok = sc <= 0x3F
    return w, np.where(ok, sc, 0), ok


HDR_BITS = np.full((16, 16), -1, np.int64)          # [p][c], -1: the step 0 -> 15 has no code
for _p in range(16):
    for _c in range(16):
        if -16 <= _c - _p <= 14:
            HDR_BITS[_p, _c] = HL[_c - _p + 16]


def step_options(typ, sub, hwin):
    """the option of every step p -> c of every (band, window index): width, scale code, allowed; each [16, NH, 16, 16]"""
    W, SC, OK = (np.zeros((16, NH, 16, 16), np.int64) for _ in range(3))
    for b in range(16):
        pm = pre_map(typ, sub, b)
        for k in range(NH):
            for pre in sorted(set(pm.tolist())):
                w, sc, allowed = options(typ, b, int(hwin[b, k]), pre)
                rows = pm == pre
                W[b, k, rows], SC[b, k, rows], OK[b, k, rows] = w, sc, allowed
    return W, SC, (OK != 0) & (HDR_BITS >= 0)[None, None]


def trellis(D, B, typ, sub, hwin, Eb):
    """every (band, h of the window, lambda) at once -> J, totD, totB [16, NH, KL] of the best end state, and the
    survivors and end states path() reads (the kernels keep totals only and walk the chosen chains a second time)"""
    F = D.shape[0]
    lam = np.array(LADDER, np.int64)
    V = np.full((16, NH, KL, 16), INF, np.int64)
    V[..., 0] = 0
    TD = np.zeros((16, NH, KL, 16), np.int64)
    TB = np.zeros((16, NH, KL, 16), np.int64)
    surv = np.zeros((F, 16, NH, KL, 16), np.int8)
    W, SC, ok = step_options(typ, sub, hwin)
    band = np.arange(16)[:, None, None, None]
    band4, k4, c4 = band, np.arange(NH)[None, :, None, None], np.arange(16)[None, None, None, :]
    for f in range(F):
        dd = D[f][band, W, SC]
        bb = B[f][band, W, SC] + np.maximum(HDR_BITS, 0)[None, None]
        md = np.maximum(dd, Eb[:, None, None, None])
        cost = lam[None, None, :, None, None] * bb[:, :, None]                                  # [16, NH, KL, p, c]
        cost += md[:, :, None]
        cost += np.where(V < INF, V, 0)[..., None]
        cost[~np.broadcast_to(ok[:, :, None] & (V < INF)[..., None], cost.shape)] = INF
        arg = cost.argmin(axis=3)                                                               # (the lowest p of a tie)
        V = np.take_along_axis(cost, arg[:, :, :, None, :], axis=3)[:, :, :, 0, :]
        TD = np.take_along_axis(TD, arg, axis=3) + dd[band4, k4, arg, c4]
        TB = np.take_along_axis(TB, arg, axis=3) + bb[band4, k4, arg, c4]
        surv[f] = arg
    # the end state: least cost, then fewer bits, then the lower code
    key = np.stack([V, TB, np.broadcast_to(np.arange(16), V.shape)], axis=-1)
    end = np.zeros(V.shape[:3], np.int64)
    for c in range(1, 16):
        cur = np.take_along_axis(key, end[..., None, None].repeat(3, axis=-1), axis=3)[:, :, :, 0, :]
        new = key[:, :, :, c, :]
        better = (new[..., 0] < cur[..., 0]) | ((new[..., 0] == cur[..., 0]) & (new[..., 1] < cur[..., 1]))
        end = np.where(better, c, end)
    g = lambda a: np.take_along_axis(a, end[..., None], axis=3)[..., 0]
    return dict(J=g(V), D=g(TD), B=g(TB), surv=surv, end=end)


def path(tr, b, k, li):
    """the code sequence [F] of one chain"""
    F = tr["surv"].shape[0]
    c = int(tr["end"][b, k, li])
    codes = np.zeros(F, np.int64)
    for f in range(F - 1, -1, -1):
        codes[f] = c
        c = int(tr["surv"][f, b, k, li, c])
    return codes


def candidates(tr, hwin, D0tot, typ, sub):
    """per lambda: each band's best h, the best band count -> list of dicts(D, bits, n, hk [16])"""
    out = []
    for li in range(KL):
        hk = np.zeros(16, np.int64)
        for b in range(16):
            best = NH - 1
            for k in range(NH - 2, -1, -1):                     # downwards in k = upwards in h: a tie stays with the lower h
                a = (int(tr["J"][b, k, li]), int(tr["B"][b, k, li]))
                if a < (int(tr["J"][b, best, li]), int(tr["B"][b, best, li])):
                    best = k
            hk[b] = best
        J = np.array([int(tr["J"][b, hk[b], li]) for b in range(16)], np.int64)
        Dn = np.array([int(tr["D"][b, hk[b], li]) for b in range(16)], np.int64)
        Bn = np.array([int(tr["B"][b, hk[b], li]) for b in range(16)], np.int64)
        nmin = 3 if (typ, sub) == (1, 0) else 1                 # both sub-type bits must be written clear: header bytes 1, 2
        best = None
        for n in range(nmin, 17):
            tot = int(J[:n].sum()) + int(D0tot[n:].sum())
            if best is None or tot < best[0]:
                best = (tot, n)
        n = best[1]
        out.append(dict(D=int(Dn[:n].sum()) + int(D0tot[n:].sum()), bits=int(Bn[:n].sum()), n=n, hk=hk))
    return out


def analyse(pcm):
    """what does not depend on the parameters: the targets and the items"""
    x = E.to_float(pcm)
    if len(x) == 0 or (len(x) + 239) // 240 > 65535:
        raise ValueError("empty stream or more than 65 535 frames")
    t = targets(E.analyse(E.frames_of(x)))
    D, B, Q0 = items(t)
    return dict(x=x, t=t, D=D, B=B, Q0=Q0, search={})


def search(an, mqe, lay):
    """the trellises of one layout of LAYOUTS under one error floor (no rate is read) -> (trellis, window, candidates)"""
    key = (float(F32(mqe)), lay)
    if key not in an["search"]:
        D0tot = an["D"][:, :, 0, 0].sum(axis=0)
        hwin = window(an["t"], lay[0])
        tr = trellis(an["D"], an["B"], lay[0], lay[1], hwin, band_floor(key[0]))
        an["search"][key] = (tr, hwin, candidates(tr, hwin, D0tot, lay[0], lay[1]))
    return an["search"][key]


def budget_bits(F, rate=None, budget_bytes=None):
    if budget_bytes is None:
        return (int(rate) * F * 240) // 31250
    return (int(budget_bytes) - 18) * 8 if budget_bytes >= 18 else -1


def allowed_variants(fmt):
    return [v for v in E.VARIANTS if fmt[0] in (-1, v[0]) and fmt[1] in (-1, v[1])]


def choose(an, fmt, mqe, budget):
    """-> dict(type, sub, ladderIndex, numBands, frameBits, budgetBits, sqErr, fits, hk)"""
    cands = []
    for vi, (typ, sub) in enumerate(E.VARIANTS):
        if (typ, sub) not in allowed_variants(fmt):
            continue
        for li, c in enumerate(search(an, mqe, (0, 0) if typ == 0 else (typ, sub))[2]):
            cands.append((c["D"], c["bits"], vi, li, c))
    fit = [x for x in cands if x[1] <= budget]
    best = min(fit, key=lambda x: x[:4]) if fit else min(cands, key=lambda x: (x[1], x[2], x[3]))
    typ, sub = E.VARIANTS[best[2]]
    return dict(type=typ, sub=sub, ladderIndex=best[3], numBands=best[4]["n"], frameBits=best[1], budgetBits=max(budget, 0),
                sqErr=best[0], fits=bool(fit), hk=best[4]["hk"])


def emit(an, ch, mqe):
    """the chosen candidate's stream bytes, its reconstruction [F, 255] and its codes [F, 16]"""
    typ, sub, n = ch["type"], ch["sub"], ch["numBands"]
    lay = (0, 0) if typ == 0 else (typ, sub)
    tr, hwin, _ = search(an, mqe, lay)
    t, D, B, Q0 = an["t"], an["D"], an["B"], an["Q0"]
    F = t.shape[0]
    codes = np.zeros((F, 16), np.int64)
    for b in range(n):
        codes[:, b] = path(tr, b, int(ch["hk"][b]), ch["ladderIndex"])
    prev = np.vstack([np.zeros((1, 16), np.int64), codes[:-1]])
    hdr = np.full(16, 0xFF, np.int64)
    cols_v, cols_n = [], []
    for b in range(n):
        hdr[b] = hwin[b, ch["hk"][b]]
        d = codes[:, b] - prev[:, b] + 16
        cols_v.append(E.HDR_CODE[d]); cols_n.append(HL[d])
    rec = np.zeros((F, 255), np.int64)
    for b in range(n):
        pre = pre_map(typ, sub, b)[prev[:, b]]
        w, sc, ref = E.interpret(typ, b, codes[:, b], int(hdr[b]), pre)
        assert (sc <= 0x3F).all()
        s0, cnt = FIRST[b], COUNT[b]
        q0 = Q0[np.arange(F)[:, None], np.arange(s0, s0 + cnt)[None, :], sc[:, None]]
        half = (1 << np.maximum(w - 1, 0))[:, None]
        q = np.where(w[:, None] > 0, np.clip(q0, -half, half - 1), 0)
        rec[:, s0:s0 + cnt] = np.where(w[:, None] > 0, recon(q, sc[:, None]), 0)
        mask = (0xFFFF >> (16 - w))[:, None]
        idx = (q + ref[:, None]) & mask
        vals, lens = idx.copy(), np.where(w[:, None] > 0, w[:, None], 0) + 0 * idx
        cb = (w >= 1) & (w <= 6)
        z = q == 0
        run = np.zeros_like(q)
        for j in range(cnt):
            run[:, j] = np.where(z[:, j], (run[:, j - 1] + 1) if j else 1, 0)
        nxt = np.hstack([z[:, 1:], np.zeros((F, 1), bool)])
        dz = z & ((run % 2) == 1) & nxt & cb[:, None]
        skip = z & ((run % 2) == 0) & cb[:, None]
        for wi in range(1, 7):
            sel = w == wi
            if sel.any():
                vals[sel] = E.SMP_CODE[wi][idx[sel]]
                lens[sel] = E.SMP_LEN[wi][idx[sel]]
                dsel = dz & sel[:, None]
                vals[dsel], lens[dsel] = E.DZ_CODE[wi], E.DZ_LEN[wi]
        lens[skip] = 0
        for j in range(cnt):
            cols_v.append(vals[:, j]); cols_n.append(lens[:, j])
    lens_all = np.stack(cols_n, 1)
    body = E.pack_bits(np.stack(cols_v, 1).ravel(), lens_all.ravel())
    assert int(lens_all.sum()) == ch["frameBits"], (int(lens_all.sum()), ch["frameBits"])
    assert int(((t - rec) ** 2).sum()) == ch["sqErr"]
    if typ != 0:
        hdr[0] |= 0x80
    hdr[1] |= (sub & 2) << 6
    hdr[2] |= (sub & 1) << 7
    return bytes([F >> 8, F & 0xFF]) + hdr.astype(np.uint8).tobytes() + body, rec, codes


def encode(an, fmt=(-1, -1), budget_bytes=None, **params):
    """-> (stream bytes, info dict, reconstruction [F, 255], codes [F, 16])"""
    p = dict(DEFAULTS, **params)
    F = an["t"].shape[0]
    budget = budget_bits(F, p["targetBitRate"], budget_bytes)
    ch = choose(an, fmt, p["maximumQuantizationError"], budget)
    s, rec, codes = emit(an, ch, p["maximumQuantizationError"])
    assert len(s) == 18 + (ch["frameBits"] + 7) // 8
    return s, ch, rec, codes


MAX_FRAME_BITS = int(sum(max(HL) + 15 * n for n in COUNT))     # every band at width 15 behind the longest delta code


def bound(n_samples):
    """the longest stream n_samples samples can encode to (0 = not encodable)"""
    nf = (n_samples + 239) // 240
    if nf == 0 or nf > 65535:
        return 0
    return 18 + (nf * MAX_FRAME_BITS + 7) // 8
