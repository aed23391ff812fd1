#!/usr/bin/env python3
"""Symbol-loop iterations of unpack94 per chunk, counted on the host from the index records: today's deal of whole bands
(dcsLaneFirstBand, rounds of 7, 9, 16, 16 ... samples) against a deal of 8-sample units (band 0, band 1, halves of the
16-sample bands; rounds of 8 samples).  No GPU.

The loop is wave-convergent, so a round costs the wavefront what its fullest lane decodes in it.  What is counted is
SAMPLES: a two-zeros code stands for two of them in one iteration, so the figures are upper bounds of the iterations, the
same bound for both deals.  A lane that meets a band without a code spends the round it starts that band in idle, as in the
kernel (the next band is set up at the top of the next round).

Chunks are the planner's own (dcs_plan_chunks2, 8 frames per wavefront, halo slots included); only chunks whose frames are
all 1994+ first sources are counted, the others keep today's deal whatever happens.

    python tools/deal_count.py [workload ...]      default: survey3_65536 realistic_65536 dcs94_65536
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import dcsexplorer_amd as D
from dcsexplorer_amd import workloads

FPW, SUB = 8, 8
SLOT_EMPTY = 0x80
BAND_SAMPLES = np.array([7, 8] + [16] * 13 + [32])


def lane_first_band(q, bpl, nb_end):
    """dcsLaneFirstBand for the 1994+ layouts"""
    return min(q * bpl + (1 if q else 0), nb_end)


def band_counts(idx, header):
    """samples to decode per band [frames, 16]: halved for a strided band, 0 for a band without a code or past nBands"""
    nb = np.minimum(idx["nBands"].astype(np.int64), 16)
    strided = (header >> 6) & 1
    cnt = BAND_SAMPLES[None, :] >> strided
    coded = (idx["bandType"] != 0) & (np.arange(16)[None, :] < nb[:, None])
    return np.where(coded, cnt, 0), BAND_SAMPLES[None, :] >> strided, nb


def deal_today(cnt, nb, serial):
    """pieces [frames, lanes, 16] and their number [frames, lanes]: whole bands, in order"""
    n = cnt.shape[0]
    pieces = np.zeros((n, SUB, 16), dtype=np.int64)
    npieces = np.zeros((n, SUB), dtype=np.int64)
    for f in range(n):
        if serial[f]:
            pieces[f, 0, :nb[f]] = cnt[f, :nb[f]]
            npieces[f, 0] = nb[f]
            continue
        bpl = max(1, (nb[f] + SUB - 1) // SUB)
        for q in range(SUB):
            b0 = lane_first_band(q, bpl, nb[f])
            b1 = lane_first_band(q + 1, bpl, nb[f]) if q + 1 < SUB else nb[f]
            pieces[f, q, :b1 - b0] = cnt[f, b0:b1]
            npieces[f, q] = b1 - b0
    return pieces, npieces


def even_deal(nb):
    """units of a frame with nb header bands -- band 0, band 1, two halves of every later band -- dealt in order to eight
    lanes, ceil(units / 8) or one fewer each: (first unit, units) per lane"""
    units = min(nb, 2) + 2 * max(nb - 2, 0)
    lo, extra = divmod(units, SUB)
    out, u = [], 0
    for q in range(SUB):
        k = lo + (1 if q < extra else 0)
        out.append((u, k))
        u += k
    return out


def unit_band(u):
    """(band, half) of unit u"""
    return (u, 0) if u < 2 else (2 + (u - 2) // 2, (u - 2) % 2)


def deal_even(cnt, full, nb, serial, today):
    """the deal of units.  A frame with all sixteen bands keeps today's deal (band 15's halves are 16 samples: units cannot
    do better than 32 there), and so does a frame in error."""
    pieces, npieces = today[0].copy(), today[1].copy()
    for f in range(cnt.shape[0]):
        if serial[f] or nb[f] >= 16:
            continue
        pieces[f] = 0
        for q, (u0, k) in enumerate(even_deal(int(nb[f]))):
            p = 0
            last = -1
            for u in range(u0, u0 + k):
                b, h = unit_band(u)
                # the second half starts where half of the band's samples (rounded up) are done
                part = cnt[f, b] if b < 2 else (0 if cnt[f, b] == 0 else (full[f, b] - full[f, b] // 2 if h == 0 else full[f, b] // 2))
                if b == last:
                    pieces[f, q, p - 1] += part        # both halves with one lane: one piece, taken over two rounds
                else:
                    pieces[f, q, p] = part
                    p += 1
                last = b
            npieces[f, q] = p
    return pieces, npieces


def iterations(pieces, npieces, chunk_of, n_chunks, round_len):
    """run the rounds: per chunk (iterations, rounds with a symbol loop)"""
    n = pieces.shape[0]
    rem = np.zeros((n, SUB), dtype=np.int64)
    nxt = np.zeros((n, SUB), dtype=np.int64)
    iters = np.zeros(n_chunks, dtype=np.int64)
    rounds = np.zeros(n_chunks, dtype=np.int64)
    fi, qi = np.meshgrid(np.arange(n), np.arange(SUB), indexing="ij")
    r = 0
    while True:
        start = (rem == 0) & (nxt < npieces)
        if not (start.any() or (rem > 0).any()):
            break
        rem = np.where(start, pieces[fi, qi, np.minimum(nxt, 15)], rem)
        nxt = nxt + start
        # (a chunk's wavefront goes round while any of its lanes has a band to start or to finish)
        busy = np.zeros(n_chunks, dtype=np.int64)
        np.maximum.at(busy, chunk_of, (start | (rem > 0)).any(axis=1).astype(np.int64))
        do = np.minimum(rem, round_len(r))
        m = np.zeros(n_chunks, dtype=np.int64)
        np.maximum.at(m, chunk_of, do.max(axis=1))
        iters += m
        rounds += busy
        rem = rem - do
        r += 1
    return iters, rounds


def count(name):
    b = workloads.build(name)
    srcs, jobs = b["srcs"], b["jobs"]
    blob = np.frombuffer(b["blob"], dtype=np.uint8)
    slots = D.plan_chunks(jobs, FPW, srcs)
    n_chunks = slots.shape[0]
    live = (slots["flags"] & SLOT_EMPTY) == 0
    job = slots["job"].astype(np.int64)
    has = live & (jobs["nSrc"][np.minimum(job, jobs.size - 1)] != 0)
    src = jobs["firstSrc"][np.minimum(job, jobs.size - 1)].astype(np.int64)
    is94 = srcs["format"][np.minimum(src, srcs.size - 1)] >= D.FMT_94_T0
    multi = jobs["nSrc"][np.minimum(job, jobs.size - 1)] > 1
    # chunks the even deal could take: every frame a single 1994+ source (or none: a silent frame)
    ok = ~((has & ~is94) | (has & multi)).any(axis=1) & has.any(axis=1)
    sel = has & ok[:, None]
    chunk_of = np.nonzero(sel)[0]
    s = src[sel]
    idx = srcs["idx"][s]
    header = blob[(srcs["streamOff"][s].astype(np.int64) + 2)[:, None] + np.arange(16)[None, :]].astype(np.int64)
    cnt, full, nb = band_counts(idx, header)
    serial = (idx["flags"] & D.IDX_SERIAL) != 0
    today = deal_today(cnt, nb, serial)
    even = deal_even(cnt, full, nb, serial, today)
    it_t, rd_t = iterations(*today, chunk_of, n_chunks, lambda r: 7 if r == 0 else 9 if r == 1 else 16)
    it_e, rd_e = iterations(*even, chunk_of, n_chunks, lambda r: 8)
    k = ok
    print("%s: %d chunks, %d all-1994+ single-source; frames there: %.1f header bands, %.1f coded, %.1f samples"
          % (name, n_chunks, int(k.sum()), nb.mean(), (cnt > 0).sum(axis=1).mean(), cnt.sum(axis=1).mean()))
    print("    today's deal  %.2f iterations per chunk (min %d, max %d) in %.2f rounds"
          % (it_t[k].mean(), it_t[k].min(), it_t[k].max(), rd_t[k].mean()))
    print("    even deal     %.2f iterations per chunk (min %d, max %d) in %.2f rounds"
          % (it_e[k].mean(), it_e[k].min(), it_e[k].max(), rd_e[k].mean()))
    print("    saved         %.2f iterations per chunk, %.2f rounds more" % ((it_t[k] - it_e[k]).mean(), (rd_e[k] - rd_t[k]).mean()))


if __name__ == "__main__":
    names = sys.argv[1:] or ["survey3_65536", "realistic_65536", "dcs94_65536"]
    if "realistic_65536" in names:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        workloads.register_recordings(np.load(os.path.join(root, "tests", "golden", "encoder_golden.npz")))
    for nm in names:
        count(nm)
