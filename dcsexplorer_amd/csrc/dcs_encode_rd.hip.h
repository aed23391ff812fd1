// dcs_encode_rd.hip.h -- the rate-distortion 1994+ encoder, included by dcs_encode.hip.
//
// dcs_encode_streams writes what the reference's DCSEncoder writes; this encoder writes the same format with header scale
// codes, band count and per-frame band-type codes of its own, from a search held to a byte budget.  What is fixed from
// outside is the decoder (DecoderImpl94, unpack94 in dcs_kernels.hip.h).  After one f32 multiply and one roundf per
// coefficient (the targets) every decision is an integer one, restated in tests/enc94rd_ref.py.
//
// These are the kernels of a family of EncRun's (EncRdFamily, dcs_encode_run.hip.h), beside the E, O and A stages:
//
//   E1  encAnalyseKernel     the 1994+ front end, unchanged (its spectrum is all that is read of it), once per stream
//   R1  encRdItemKernel      a block per STREAM-frame, the frame's targets and their nearest sample values in LDS: for every
//                            band, width 1..15 and scale code 0..63 the squared error against the decoder's word and the exact
//                            sample bits (width 0: the band's energy), 128 KB a frame; the bands' peaks and energies per stream
//   R2  encRdTrellisKernel<false>  a 16-lane row per chain (job, layout, band, header code of the window, lambda), a lane per
//                            state = the previous frame's band-type code; the sixteen predecessors by row-wide cross-lane
//                            reads, the next frame's items loaded before this frame's step; totals only
//   R3  encRdChooseKernel    a block per job: per (layout, lambda) each band's best header code and the best band count, then
//                            the least error within the job's budget
//   R4  encRdTrellisKernel<true>   the chosen sixteen chains of a job again, survivors kept; encRdBackKernel walks them back
//   R5  encRdBitsKernel, encRdOffsetKernel   the frames' bit counts and offsets
//   R6  encRdHeadKernel, encRdPackKernel     frame count, header, and per job-frame a lane per band: delta code and samples,
//                            quantised as R1 quantised them (integers, clamped, never masked), OR-ed into big-endian words

namespace {

// the decoder's frame-buffer word for sample value q at scale factor `scale` (mixAdd on a zero accumulator, at M0)
__device__ __forceinline__ int rdRecon(int q, int scale)
{
    const uint32_t low = static_cast<uint32_t>(q * scale) & 0xFFFFu;
    const int sx = static_cast<int16_t>(low);
    const uint32_t acc = low + static_cast<uint32_t>(sx * static_cast<int>(kRdM0));
    return static_cast<int16_t>(acc >> 16);
}

__device__ __forceinline__ int rdTarget(const float *frame, int k)
{
    const float r = roundf(frame[k] * kRdK);
    return static_cast<int>(fminf(fmaxf(r, -32768.0f), 32767.0f));
}

// the sample value whose word is nearest to t at one scale code: the estimate (|t| * rcp) >> 24 with -1 .. +2 added (the
// word is floor(q * scale * (M0 + 1) / 65536) in magnitude, so the nearest lies there), the smaller magnitude first,
// replaced on strictly less
__device__ __forceinline__ int rdNearest(int t, int scale, uint32_t rcp, int qmax)
{
    const int s = t > 0 ? 1 : t < 0 ? -1 : 0;
    const int est = static_cast<int>((static_cast<unsigned long long>(static_cast<uint32_t>(abs(t))) * rcp) >> 24);
    int best = 0, berr = 0;
#pragma unroll
    for (int d = -1 ; d <= 2 ; ++d)
    {
        const int q = min(max(s * (est + d), -qmax), qmax);
        const int err = abs(t - rdRecon(q, scale));
        if (d == -1 || err < berr) { best = q; berr = err; }
    }
    return best;
}

__device__ __forceinline__ int rdClampWidth(int q, int w) { return min(max(q, -(1 << (w - 1))), (1 << (w - 1)) - 1); }

// the header scale code at index k of a band's window: from the band's peak over the stream
__device__ __forceinline__ int rdHeaderCode(const EncTabs &T, uint32_t peak, int typ, int k)
{
    const int pk = max(static_cast<int>(peak), 1);
    int top = 0;
    for (int j = 0 ; j < 64 ; ++j)
        top += T.scale[j] < pk ? 1 : 0;
    return min(max(top - (typ ? kRdHBase1 : kRdHBase0) - kRdHStep * k, 0), 63);
}

// R1: a block per stream-frame
__global__ __launch_bounds__(256) void encRdItemKernel(const EncTabs *__restrict__ Tp, const EncRdTabs *__restrict__ Rp,
    const float *__restrict__ spec, const uint32_t *__restrict__ frameStream, unsigned long long *__restrict__ items,
    uint32_t *__restrict__ peak, unsigned long long *__restrict__ d0tot)
{
    const EncTabs &T = *Tp;
    const EncRdTabs &R = *Rp;
    __shared__ int st[256];
    __shared__ int16_t sq[255 * 64];
    __shared__ int sScale[64], sQmax[64];
    __shared__ uint32_t sRcp[64];
    __shared__ uint8_t sLen[7][64], sDz[7];
    __shared__ int sFirst[16], sCount[16];
    const int tid = threadIdx.x;
    const uint32_t f = blockIdx.x;
    st[tid] = tid < 255 ? rdTarget(spec + static_cast<size_t>(f) * 256, tid) : 0;
    if (tid < 64) { sScale[tid] = T.scale[tid]; sQmax[tid] = R.qmax[tid]; sRcp[tid] = R.rcp[tid]; }
    for (int i = tid ; i < 7 * 64 ; i += 256)
        (&sLen[0][0])[i] = (&T.smpLen[0][0])[i];
    if (tid < 7) sDz[tid] = T.dzLen[tid];
    if (tid < 16) { sFirst[tid] = T.first[tid]; sCount[tid] = T.count[tid]; }
    __syncthreads();
    for (int i = tid ; i < 255 * 64 ; i += 256)
    {
        const int e = i & 63;
        sq[i] = static_cast<int16_t>(rdNearest(st[i >> 6], sScale[e], sRcp[e], sQmax[e]));
    }
    __syncthreads();
    unsigned long long *out = items + static_cast<size_t>(f) * kRdItemsPerFrame;
    for (int i = tid ; i < static_cast<int>(kRdItemsPerFrame) ; i += 256)
    {
        const int b = i >> 10, w = (i >> 6) & 15, e = i & 63;
        const int s0 = sFirst[b], n = sCount[b];
        unsigned long long D = 0;
        uint32_t bits = 0;
        if (w == 0)
        {
            for (int j = 0 ; j < n ; ++j)
                D += static_cast<unsigned long long>(static_cast<uint32_t>(st[s0 + j] * st[s0 + j]));
        }
        else
        {
            const int scale = sScale[e], ref = 1 << (w - 1);
            const bool book = w <= 6;
            bool pend = false;                  // the sample before was a zero still coded alone
            for (int j = 0 ; j < n ; ++j)
            {
                const int q = rdClampWidth(sq[(s0 + j) * 64 + e], w);
                const int d = st[s0 + j] - rdRecon(q, scale);
                D += static_cast<unsigned long long>(static_cast<uint32_t>(d) * static_cast<uint32_t>(d));
                if (!book)
                    continue;
                if (q == 0 && pend) { bits += static_cast<uint32_t>(sDz[w]) - sLen[w][ref]; pend = false; }
                else { bits += sLen[w][q + ref]; pend = q == 0; }
            }
            if (!book)
                bits = static_cast<uint32_t>(w * n);
        }
        out[i] = D | (static_cast<unsigned long long>(bits) << 48);
        if (w == 0 && e == 0)
        {
            int pk = 0;
            for (int j = 0 ; j < n ; ++j)
                pk = max(pk, abs(st[s0 + j]));
            const uint32_t s = frameStream[f];
            atomicMax(&peak[s * 16 + b], static_cast<uint32_t>(pk));
            atomicAdd(&d0tot[s * 16 + b], D);
        }
    }
}

// R2 (SURV = false): grid (jobs of the group) x (rows of a job / 16), a row per chain; totals to tot[job][layout][band][k][lambda].
// R4 (SURV = true): grid (jobs of the group), row = band: the job's chosen chain of that band, every step's predecessor to
// surv[job-frame][band][state] and the end state to endState[job][band].
template <bool SURV>
__global__ __launch_bounds__(256) void encRdTrellisKernel(const EncTabs *__restrict__ Tp, const EncRdTabs *__restrict__ Rp,
    const unsigned long long *__restrict__ items, const uint32_t *__restrict__ peak, const unsigned long long *__restrict__ floorE,
    const EncJob *__restrict__ jobs, const EncSet *__restrict__ sets, EncRdTot *__restrict__ tot,
    const EncRdChoice *__restrict__ choice, uint8_t *__restrict__ surv, uint8_t *__restrict__ endState)
{
    const EncTabs &T = *Tp;
    __shared__ uint8_t sHL[32];
    const int tid = threadIdx.x, c = tid & 15;
    if (tid < 31) sHL[tid] = T.hdrLen[tid];
    __syncthreads();
    const uint32_t ji = SURV ? blockIdx.x : blockIdx.x / (kRdRowsPerJob / 16);
    const EncJob job = jobs[ji];
    int v, b, k, li;
    if (SURV)
    {
        const EncRdChoice ch = choice[ji];
        b = tid >> 4;
        if (b >= ch.numBands)
            return;
        v = ch.variant < 2 ? 0 : ch.variant - 1;
        k = ch.hk[b];
        li = ch.ladderIndex;
    }
    else
    {
        const uint32_t row = (blockIdx.x % (kRdRowsPerJob / 16)) * 16 + (tid >> 4);
        v = static_cast<int>(row / kRdRowsPerLayout);
        if (((sets[job.set].vmask >> v) & 1u) == 0)
            return;
        const uint32_t r = row % kRdRowsPerLayout;
        b = static_cast<int>(r / (kRdNH * kRdKL));
        k = static_cast<int>((r / kRdKL) % kRdNH);
        li = static_cast<int>(r % kRdKL);
    }
    const int typ = v ? 1 : 0;
    const int h = rdHeaderCode(T, peak[job.stream * 16 + b], typ, k);
    const unsigned long long lam = Rp->ladder[li], eb = floorE[static_cast<size_t>(job.set) * 16 + b];
    const bool preBand = typ == 1 && b < 3;
    const int npre = !preBand ? 1 : v == 1 ? 2 : 5;
    // the pre-adjust of every previous code p (kPreAdjSub0 / kPreAdjSub3, at most 4), four bits each: the unrolled loop below
    // takes its field with a constant shift and picks the lane's item by compares, so nothing is indexed by a variable
    unsigned long long preOf = 0;
    if (preBand)
        for (int p = 0 ; p < 16 ; ++p)
            preOf |= static_cast<unsigned long long>(T.preAdj[v - 1][p]) << (4 * p);
    const int cls = b < 3 ? 0 : b < 6 ? 1 : 2;
    const int w = c == 0 ? 0 : typ == 0 ? c : T.xw[cls][c];
    const int e0 = c == 0 ? 0 : typ == 0 ? h : h + T.xa[cls][c];
    const size_t rowBase = (static_cast<size_t>(b) * 16 + w) * 64;

    unsigned long long V = c == 0 ? 0 : kRdInf, TD = 0;
    uint32_t TB = 0;
    unsigned long long it[5], nx[5];
    auto load = [&](uint32_t f, unsigned long long *dst)
    {
        const unsigned long long *p = items + static_cast<size_t>(job.specFirst + f) * kRdItemsPerFrame + rowBase;
#pragma unroll
        for (int j = 0 ; j < 5 ; ++j)
        {
            const int e = c == 0 ? 0 : e0 + j;
            dst[j] = (j < npre && e <= 63) ? p[e] : kRdNoItem;
        }
    };
    load(0, it);
    for (uint32_t f = 0 ; f < job.nFrames ; ++f)
    {
        if (f + 1 < job.nFrames)
            load(f + 1, nx);
        unsigned long long best = kRdInf, bD = 0;
        uint32_t bB = 0;
        int bp = 0;
#pragma unroll
        for (int p = 0 ; p < 16 ; ++p)
        {
            const unsigned long long Vp = __shfl(V, p, 16);
            const uint32_t pre = static_cast<uint32_t>(preOf >> (4 * p)) & 15u;
            unsigned long long item = it[0];
#pragma unroll
            for (int j = 1 ; j < 5 ; ++j)
                item = pre == static_cast<uint32_t>(j) ? it[j] : item;
            const uint32_t nb = static_cast<uint32_t>(sHL[c - p + 16]) + static_cast<uint32_t>(item >> 48);
            const unsigned long long D = item & kRdDMask;
            const unsigned long long cost = Vp + (D > eb ? D : eb) + lam * nb;
            const bool ok = Vp < kRdInf && item != kRdNoItem && !(p == 0 && c == 15);
            if (ok && cost < best) { best = cost; bp = p; bD = D; bB = nb; }          // (the lowest p of a tie)
        }
        TD = __shfl(TD, bp, 16) + bD;
        TB = __shfl(TB, bp, 16) + bB;
        V = best;
        if (SURV)
            surv[(static_cast<size_t>(job.firstFrame) + f) * 256 + b * 16 + c] = static_cast<uint8_t>(bp);
#pragma unroll
        for (int j = 0 ; j < 5 ; ++j)
            it[j] = nx[j];
    }
    // the end state: least cost, then fewer bits, then the lower code
    int wc = c;
#pragma unroll
    for (int off = 8 ; off >= 1 ; off >>= 1)
    {
        const unsigned long long oV = __shfl_xor(V, off, 16), oD = __shfl_xor(TD, off, 16);
        const uint32_t oB = __shfl_xor(TB, off, 16);
        const int oc = __shfl_xor(wc, off, 16);
        if (oV < V || (oV == V && (oB < TB || (oB == TB && oc < wc)))) { V = oV; TD = oD; TB = oB; wc = oc; }
    }
    if (c != 0)
        return;
    if (SURV)
        endState[ji * 16 + b] = static_cast<uint8_t>(wc);
    else
        tot[(((static_cast<size_t>(ji) * 3 + v) * 16 + b) * kRdNH + k) * kRdKL + li] = EncRdTot{ V, TD, TB, 0 };
}

// the chosen chains walked back: a thread per (job, band); bands the header cuts keep code 0 (codes is zeroed before)
__global__ __launch_bounds__(64) void encRdBackKernel(const EncJob *__restrict__ jobs, const EncRdChoice *__restrict__ choice,
    const uint8_t *__restrict__ surv, const uint8_t *__restrict__ endState, uint32_t n, uint8_t *__restrict__ codes)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x, ji = i >> 4, b = i & 15;
    if (ji >= n || static_cast<int>(b) >= choice[ji].numBands)
        return;
    const EncJob job = jobs[ji];
    int c = endState[ji * 16 + b];
    for (uint32_t f = job.nFrames ; f-- > 0 ; )
    {
        const size_t jf = static_cast<size_t>(job.firstFrame) + f;
        codes[jf * 16 + b] = static_cast<uint8_t>(c);
        c = surv[jf * 256 + b * 16 + c];
    }
}

// R3: a block per job of the group, a thread per (layout, lambda); thread 0 picks within the job's budget
__global__ __launch_bounds__(256) void encRdChooseKernel(const EncRdTot *__restrict__ tot, const unsigned long long *__restrict__ d0tot,
    const EncJob *__restrict__ jobs, const EncSet *__restrict__ sets, const long long *__restrict__ budget,
    EncRdChoice *__restrict__ choice)
{
    __shared__ unsigned long long sD[3 * kRdKL], sBits[3 * kRdKL], sSuf[17];
    __shared__ int sN[3 * kRdKL];
    __shared__ uint8_t sHk[3 * kRdKL][16];
    const int tid = threadIdx.x;
    const uint32_t ji = blockIdx.x;
    const EncJob job = jobs[ji];
    const EncSet set = sets[job.set];
    if (tid == 0)
    {
        sSuf[16] = 0;
        for (int b = 15 ; b >= 0 ; --b)
            sSuf[b] = sSuf[b + 1] + d0tot[job.stream * 16 + b];
    }
    __syncthreads();
    if (tid < 3 * kRdKL)
    {
        const int v = tid / kRdKL, li = tid % kRdKL;
        const int nmin = v == 1 ? 3 : 1;        // (1, 0): header bytes 1 and 2 carry the sub-type bits, both clear
        unsigned long long preJ = 0, preD = 0, preB = 0, bestTot = 0, bD = 0, bBits = 0;
        int bn = 0;
        if ((set.vmask >> v) & 1u)
            for (int b = 0 ; b < 16 ; ++b)
            {
                const EncRdTot *tb = tot + (((static_cast<size_t>(ji) * 3 + v) * 16 + b) * kRdNH) * kRdKL + li;
                int bk = kRdNH - 1;
                EncRdTot bt = tb[static_cast<size_t>(bk) * kRdKL];
                for (int k = kRdNH - 2 ; k >= 0 ; --k)             // upwards in h: a tie stays with the lower h
                {
                    const EncRdTot t = tb[static_cast<size_t>(k) * kRdKL];
                    if (t.J < bt.J || (t.J == bt.J && t.bits < bt.bits)) { bt = t; bk = k; }
                }
                sHk[tid][b] = static_cast<uint8_t>(bk);
                preJ += bt.J; preD += bt.D; preB += bt.bits;
                const int n = b + 1;
                const unsigned long long totJ = preJ + sSuf[n];
                if (n >= nmin && (bn == 0 || totJ < bestTot)) { bestTot = totJ; bn = n; bD = preD + sSuf[n]; bBits = preB; }
            }
        sD[tid] = bD; sBits[tid] = bBits; sN[tid] = bn;
    }
    __syncthreads();
    if (tid != 0)
        return;
    const long long cap = budget[ji];
    int best = -1, least = -1, bestVar = 0, leastVar = 0;
    for (int var = 0 ; var < 4 ; ++var)
    {
        if (((set.cmask >> var) & 1u) == 0)
            continue;
        const int v = var < 2 ? 0 : var - 1;
        for (int li = 0 ; li < kRdKL ; ++li)
        {
            const int k = v * kRdKL + li;
            if (least < 0 || sBits[k] < sBits[least]) { least = k; leastVar = var; }
            if (cap >= 0 && sBits[k] <= static_cast<unsigned long long>(cap)
                && (best < 0 || sD[k] < sD[best] || (sD[k] == sD[best] && sBits[k] < sBits[best]))) { best = k; bestVar = var; }
        }
    }
    const int win = best >= 0 ? best : least;
    EncRdChoice ch = { best >= 0 ? bestVar : leastVar, win % kRdKL, sN[win], best >= 0 ? 1 : 0, sBits[win], sD[win], {} };
    for (int b = 0 ; b < 16 ; ++b)
        ch.hk[b] = sHk[win][b];
    choice[ji] = ch;
}

// what code c after code p means in band b of a job's chosen layout: width, scale code, and the delta code's length
struct EncRdOpt { int w, e; };
__device__ __forceinline__ EncRdOpt rdOption(const EncTabs &T, int variant, int b, int c, int p, int h)
{
    if (c == 0)
        return EncRdOpt{ 0, 0 };
    if (variant < 2)
        return EncRdOpt{ c, h };
    const int cls = b < 3 ? 0 : b < 6 ? 1 : 2;
    return EncRdOpt{ T.xw[cls][c], (h + T.xa[cls][c] + (b < 3 ? T.preAdj[variant - 2][p] : 0)) & 63 };     // (a chosen step's is at most 0x3F)
}

// one band of one job-frame: its delta code's length and its sample bits
__device__ __forceinline__ void rdBandBits(const EncTabs &T, const unsigned long long *__restrict__ items, const uint8_t *__restrict__ codes,
    const uint32_t *__restrict__ peak, const EncJob &job, const EncRdChoice &ch, uint32_t jf, int b, uint32_t *hl, uint32_t *smp)
{
    const int c = codes[static_cast<size_t>(jf) * 16 + b], p = jf > job.firstFrame ? codes[static_cast<size_t>(jf - 1) * 16 + b] : 0;
    const int h = rdHeaderCode(T, peak[job.stream * 16 + b], ch.variant < 2 ? 0 : 1, ch.hk[b]);
    const EncRdOpt o = rdOption(T, ch.variant, b, c, p, h);
    *hl = T.hdrLen[c - p + 16];
    *smp = c == 0 ? 0u : static_cast<uint32_t>(items[static_cast<size_t>(encSpecFrame(job, jf)) * kRdItemsPerFrame
                                                       + (static_cast<size_t>(b) * 16 + o.w) * 64 + o.e] >> 48);
}

// R5: a thread per job-frame of the group
__global__ __launch_bounds__(64) void encRdBitsKernel(const EncTabs *__restrict__ Tp, const unsigned long long *__restrict__ items,
    const uint32_t *__restrict__ peak, const uint32_t *__restrict__ frameJob, const EncJob *__restrict__ jobs,
    const EncRdChoice *__restrict__ choice, const uint8_t *__restrict__ codes, uint32_t JF, uint32_t *__restrict__ frameBits)
{
    const uint32_t jf = blockIdx.x * 64 + threadIdx.x;
    if (jf >= JF)
        return;
    const uint32_t ji = frameJob[jf];
    const EncJob job = jobs[ji];
    const EncRdChoice ch = choice[ji];
    uint32_t bits = 0;
    for (int b = 0 ; b < ch.numBands ; ++b)
    {
        uint32_t hl, smp;
        rdBandBits(*Tp, items, codes, peak, job, ch, jf, b, &hl, &smp);
        bits += hl + smp;
    }
    frameBits[jf] = bits;
}

// a block per job: the exclusive scan of its frames' bits
__global__ __launch_bounds__(256) void encRdOffsetKernel(const EncJob *__restrict__ jobs, const uint32_t *__restrict__ frameBits,
    uint32_t *__restrict__ frameOff)
{
    __shared__ uint32_t scan[256];
    __shared__ uint32_t carry;
    const EncJob s = jobs[blockIdx.x];
    const int t = threadIdx.x;
    if (t == 0)
        carry = 0;
    __syncthreads();
    for (uint32_t j0 = 0 ; j0 < s.nFrames ; j0 += 256)
    {
        const uint32_t j = j0 + t;
        const uint32_t x = j < s.nFrames ? frameBits[s.firstFrame + j] : 0;
        scan[t] = x;
        __syncthreads();
        for (int w = 1 ; w < 256 ; w <<= 1)
        {
            const uint32_t y = t >= w ? scan[t - w] : 0;
            __syncthreads();
            scan[t] += y;
            __syncthreads();
        }
        if (j < s.nFrames)
            frameOff[s.firstFrame + j] = carry + scan[t] - x;
        __syncthreads();
        if (t == 255)
            carry += scan[255];
        __syncthreads();
    }
}

// the frame count and the sixteen header bytes of each job of the group; bands from numBands on are cut with 0xFF
__global__ __launch_bounds__(64) void encRdHeadKernel(const EncTabs *__restrict__ Tp, const uint32_t *__restrict__ peak,
    const EncJob *__restrict__ jobs, const EncRdChoice *__restrict__ choice, const uint64_t *__restrict__ outOff, uint32_t n,
    uint32_t *__restrict__ W)
{
    const uint32_t si = blockIdx.x * 64 + threadIdx.x;
    if (si >= n)
        return;
    const EncJob job = jobs[si];
    const EncRdChoice ch = choice[si];
    const int typ = ch.variant < 2 ? 0 : 1, sub = (ch.variant & 1) ? 3 : 0;
    const uint64_t at = outOff[si] * 8;
    encPut(W, at, job.nFrames, 16);
    for (int b = 0 ; b < 16 ; ++b)
    {
        uint32_t hb = b < ch.numBands ? static_cast<uint32_t>(rdHeaderCode(*Tp, peak[job.stream * 16 + b], typ, ch.hk[b])) : 0xFFu;
        if (b == 0 && typ != 0) hb |= 0x80u;
        if (b == 1) hb |= static_cast<uint32_t>((sub & 2) << 6);
        if (b == 2) hb |= static_cast<uint32_t>((sub & 1) << 7);
        encPut(W, at + 16 + 8 * b, hb, 8);
    }
}

// R6: a block per job-frame, a lane per band: where its delta code and its samples go, then the code and the samples
__global__ __launch_bounds__(64) void encRdPackKernel(const EncTabs *__restrict__ Tp, const EncRdTabs *__restrict__ Rp,
    const float *__restrict__ spec, const unsigned long long *__restrict__ items, const uint32_t *__restrict__ peak,
    const uint32_t *__restrict__ frameJob, const EncJob *__restrict__ jobs, const EncRdChoice *__restrict__ choice,
    const uint8_t *__restrict__ codes, const uint32_t *__restrict__ frameOff, const uint64_t *__restrict__ outOff,
    uint32_t *__restrict__ W)
{
    const EncTabs &T = *Tp;
    const uint32_t jf = blockIdx.x, si = frameJob[jf];
    const int b = threadIdx.x;
    const EncJob job = jobs[si];
    const EncRdChoice ch = choice[si];
    if (b >= ch.numBands)
        return;
    uint32_t hdrPos = 0, hdrAll = 0, smpPos = 0, myHl = 0;
    for (int j = 0 ; j < ch.numBands ; ++j)
    {
        uint32_t hl, smp;
        rdBandBits(T, items, codes, peak, job, ch, jf, j, &hl, &smp);
        hdrAll += hl;
        if (j < b) { hdrPos += hl; smpPos += smp; }
        if (j == b) myHl = hl;
    }
    const uint64_t base = (outOff[si] + 18) * 8 + frameOff[jf];
    const int c = codes[static_cast<size_t>(jf) * 16 + b], p = jf > job.firstFrame ? codes[static_cast<size_t>(jf - 1) * 16 + b] : 0;
    encPut(W, base + hdrPos, T.hdrCode[c - p + 16], static_cast<int>(myHl));
    if (c == 0)
        return;
    const int h = rdHeaderCode(T, peak[job.stream * 16 + b], ch.variant < 2 ? 0 : 1, ch.hk[b]);
    const EncRdOpt o = rdOption(T, ch.variant, b, c, p, h);
    const int scale = T.scale[o.e], qmax = Rp->qmax[o.e], w = o.w, n = T.count[b];
    const uint32_t rcp = Rp->rcp[o.e];
    const float *frame = spec + static_cast<size_t>(encSpecFrame(job, jf)) * 256 + T.first[b];
    const bool book = w <= 6;
    const int ref = book ? 1 << (w - 1) : 0, mask = 0xFFFF >> (16 - w);
    uint64_t pos = base + hdrAll + smpPos;
    int q = rdClampWidth(rdNearest(rdTarget(frame, 0), scale, rcp, qmax), w);
    for (int i = 0 ; i < n ; ++i)
    {
        const int qn = i + 1 < n ? rdClampWidth(rdNearest(rdTarget(frame, i + 1), scale, rcp, qmax), w) : 1;
        uint32_t code;
        int len;
        if (book && q == 0 && qn == 0)
        {
            code = T.dzCode[w]; len = T.dzLen[w];
            ++i;
            q = i + 1 < n ? rdClampWidth(rdNearest(rdTarget(frame, i + 1), scale, rcp, qmax), w) : 1;
        }
        else
        {
            const int vv = (q + ref) & mask;
            code = book ? T.smpCode[w][vv] : static_cast<uint32_t>(vv);
            len = book ? T.smpLen[w][vv] : w;
            q = qn;
        }
        encPut(W, pos, code, len);
        pos += static_cast<uint64_t>(len);
    }
}

}  // namespace
