"""Plain numpy / Python-int restatements of what dcs_encode_sweep measures and dcs_encode_fit chooses, written from the
text of include/dcs_hip.h ("Sweeping parameters and fitting a byte budget"), not from the library's code."""
import numpy as np

LAG = 16                    # the decoded signal trails the source by the frames' overlap
RATES = (256000, 192000, 128000, 96000, 64000, 48000)          # the bit rates of the golden and the end-to-end cases


def quantise(x):
    """q[k] = clamp(rint(x[k] * 32768), -32768, 32767), ties to even; int16 input is its own q"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.int64)
    return np.clip(np.rint(x.astype(np.float32) * np.float32(32768.0)), -32768, 32767).astype(np.int64)


def sums(q, d):
    """the four numbers for q against d, equally long int64 arrays, as Python ints"""
    q = [int(v) for v in q]
    d = [int(v) for v in d]
    return dict(sumSrcSq=sum(a * a for a in q), sumDecSq=sum(b * b for b in d), sumCross=sum(a * b for a, b in zip(q, d)),
                peakErr=max([abs(b - a) for a, b in zip(q, d)] or [0]))


def measure(x, decoded, lag=LAG):
    """x: the source (float32 in [-1, 1] or int16); decoded: int16 [nFrames + 1, 240] of a fresh decoder at unity.
    -> dict(nCompared, sumSrcSq, sumDecSq, sumCross, peakErr), all Python ints"""
    q = quantise(x)
    n = len(q)
    d = np.asarray(decoded).reshape(-1).astype(np.int64)
    assert len(d) >= n + lag, "the decode must run one frame past the stream"
    return dict(nCompared=n, **sums(q, d[lag:lag + n]))


def sq_err(m):
    return m["sumDecSq"] - 2 * m["sumCross"] + m["sumSrcSq"]


def fit(n_bytes, sq_err_, budget):
    """tables [nStreams][nSets] of ints, sets most preferred first -> (status, choice list, total); status 0 or -5"""
    n, k = len(n_bytes), len(n_bytes[0])
    col = [sum(int(n_bytes[i][r]) for i in range(n)) for r in range(k)]
    fits = [r for r in range(k) if col[r] <= budget]
    if not fits:
        r = min(range(k), key=lambda c: (col[c], c))
        return -5, [r] * n, col[r]
    r = fits[0]
    choice, total = [r] * n, col[r]
    for i in sorted(range(n), key=lambda i: (-int(sq_err_[i][r]), i)):
        for c in range(r):
            if int(sq_err_[i][c]) < int(sq_err_[i][r]) and total - int(n_bytes[i][r]) + int(n_bytes[i][c]) <= budget:
                total += int(n_bytes[i][c]) - int(n_bytes[i][r])
                choice[i] = c
                break
    return 0, choice, total
