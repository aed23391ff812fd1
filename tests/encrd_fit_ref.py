"""The allocator of DESIGN.md 10.13, restated in plain Python integers (test infrastructure): curves of (size, D) candidates ->
one allotment per job under a shared total, and the fit calls over the restatements of the two rate-distortion encoders
(enc94rd_ref, enc93rd_ref).  Nothing here is shared with the library."""
from fractions import Fraction

MAX_POINTS = 168


def hull(points, cap=None):
    """steps 1 to 3 for one job: [(size, D)] in candidate order -> (vertices [(size, D)], pinned)"""
    kept = [p for p in points if cap is None or p[0] <= cap]
    if not kept:
        return [min(points, key=lambda p: p[0])], True       # (min keeps the first of the smallest)
    stair = []
    for s, d in sorted(kept):
        if not stair or d < stair[-1][1]:
            stair.append((s, d))
    h = []
    for s, d in stair:
        while len(h) >= 2:
            (sa, da), (sb, db) = h[-2], h[-1]
            if (da - db) * (s - sb) > (db - d) * (sb - sa):     # into the middle strictly steeper than out of it
                break
            h.pop()
        h.append((s, d))
    return h, False


def allot(curves, total, caps=None):
    """-> (allotments, record dict, hulls)"""
    hulls = [hull(list(c), None if caps is None else int(caps[j]))[0] for j, c in enumerate(curves)]
    at = [0] * len(curves)
    base = sum(h[0][0] for h in hulls)
    steps = []
    for j, h in enumerate(hulls):
        for i in range(1, len(h)):
            steps.append((Fraction(h[i - 1][1] - h[i][1], h[i][0] - h[i - 1][0]), j, i - 1))
    fits = base <= total
    taken = 0
    if fits:
        remaining = total - base
        stopped = set()
        for _, j, i in sorted(steps, key=lambda t: (-t[0], t[1], t[2])):
            if j in stopped:
                continue
            ds = hulls[j][i + 1][0] - hulls[j][i][0]
            if ds > remaining:
                stopped.add(j)
                continue
            assert at[j] == i
            remaining -= ds
            at[j] = i + 1
            taken += 1
    sizes = [h[k][0] for h, k in zip(hulls, at)]
    rec = dict(totalBytes=total, leastBytes=base, usedBytes=sum(sizes), sqErr=sum(h[k][1] for h, k in zip(hulls, at)),
               nSteps=len(steps), stepsTaken=taken, fits=int(fits))
    return sizes, rec, hulls


def record_tuple(rec):
    """a record dict, or an ENCODE_RD_FIT_INFO_DTYPE record, as a tuple"""
    return tuple(int(rec[k]) for k in ("totalBytes", "leastBytes", "usedBytes", "sqErr", "nSteps", "stepsTaken", "fits"))


# ---------------------------------------------------------------------------------------- the fit calls over the restatements

def curve94(R, an, fmt, mqe):
    """the candidates of one 1994+ job in the library's order: layout (0, 0), (1, 0), (1, 3), each by ladder index"""
    allowed = R.allowed_variants(fmt)
    out = []
    for lay in [(0, 0), (1, 0), (1, 3)]:
        if not any((v if v[0] else (0, 0)) == lay for v in allowed):
            continue
        for c in R.search(an, mqe, lay)[2]:
            out.append((18 + (int(c["bits"]) + 7) // 8, int(c["D"])))
    return out


def curve93(R, an, mqe):
    sr = R.search(an, mqe)
    return [(18 + (int(sr["bits"][li]) + 7) // 8, int(sr["D"][li])) for li in range(R.KL)]


def budgets(sizes, caps):
    """what each job's per-stream call is given: its allotment, or its cap where even its smallest candidate is beyond it"""
    return [s if caps is None else min(s, int(caps[j])) for j, s in enumerate(sizes)]


def fit94(R, ans, total, fmt=(-1, -1), caps=None, **params):
    """-> (streams, info dicts, record dict, allotments)"""
    p = dict(R.DEFAULTS, **params)
    mqe = p["maximumQuantizationError"]
    sizes, rec, _ = allot([curve94(R, an, fmt, mqe) for an in ans], total, caps)
    res = [R.encode(an, fmt, b, **params) for an, b in zip(ans, budgets(sizes, caps))]
    rec["sqErr"] = sum(r[1]["sqErr"] for r in res)
    return [r[0] for r in res], [r[1] for r in res], rec, sizes


def fit93(R, ans, total, caps=None, **params):
    p = dict(R.DEFAULTS, **params)
    mqe = p["maximumQuantizationError"]
    sizes, rec, _ = allot([curve93(R, an, mqe) for an in ans], total, caps)
    res = [R.encode(an, b, **params) for an, b in zip(ans, budgets(sizes, caps))]
    rec["sqErr"] = sum(r[1]["sqErr"] for r in res)
    return [r[0] for r in res], [r[1] for r in res], rec, sizes
