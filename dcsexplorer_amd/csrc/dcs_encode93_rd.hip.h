// dcs_encode93_rd.hip.h -- the rate-distortion OS93 Type-0 encoder, included by dcs_encode.hip.
//
// dcs_encode93_streams writes what the reference's DCSEncoder writes; this encoder writes the same layout (OS93 Type 0, one
// bit stream under 0x9301 and 0x9302) with header scale codes, band count and per-frame band options of its own, from a
// search held to a byte budget.  What is fixed from outside is the decoder (DecoderImpl93::DecompressFrame; unpack93 in
// dcs_kernels.hip.h).  The decoder's state is reset at every frame, so the trellis runs over the BANDS of one frame and the
// frames are independent.  After one f32 multiply and one roundf per coefficient (the targets) every decision is an integer
// one, restated in tests/enc93rd_ref.py.
//
// These are the kernels of a family of EncRun's (Enc93RdFamily, dcs_encode_run.hip.h), beside the E, O, A and R stages:
//
//   E1  encAnalyseKernel       the front end, unchanged (its spectrum is all that is read of it), once per stream
//   S1  enc93RdItemKernel      a block per STREAM-frame, the frame's targets and their nearest values in LDS: per band, scale
//                              code and option (zero, direct 1..15) the squared error against the decoder's word, 128 KB a
//                              frame, and per band and scale code what the delta options need of the unclamped values
//   S2  enc93RdProxyKernel     per (job, band, scale code, lambda) the sum over the frames of the least step cost over the zero
//                              and direct options; a thread walks 64 job-frames and adds its sums by integer atomics
//   S3  enc93RdHeaderKernel    a block per job, a thread per lambda: each band's scale code and the band count
//   S4  enc93RdTrellisKernel<false>  a 32-lane group per (job-frame, lambda), a lane per state, the bands in turn; the
//                              predecessors by group-wide cross-lane reads; totals per (job, lambda) by integer atomics
//   S5  enc93RdChooseKernel    a thread per job: the least error within the job's budget
//   S6  enc93RdTrellisKernel<true>   the chosen lambda again, each lane's survivors packed into two registers and walked
//                              back by cross-lane reads: the frame's states and its bits
//   S7  encRdOffsetKernel      (dcs_encode_rd.hip.h) the frames' offsets
//   S8  enc93RdHeadKernel, enc93RdPackKernel   frame count and header; per job-frame a lane per band: the band-type code and
//                              the values, quantised as S1 quantised them (integers, clamped, never masked)

namespace {

// the decoder's frame-buffer word for sample value q at scale factor `scale` (AddOutput on a zero accumulator, at m0)
__device__ __forceinline__ int rd93Recon(int q, int scale, uint32_t m0)
{
    const uint32_t low = static_cast<uint32_t>(q * scale) & 0xFFFFu;
    const int sx = static_cast<int16_t>(low);
    const uint32_t acc = low + static_cast<uint32_t>(sx * static_cast<int>(m0));
    return static_cast<int16_t>(acc >> 16);
}

// The target of sample k: the spectrum NEGATED.  The OS93 transform returns the PCM of a frame buffer with its polarity
// turned (the decode of a reference-equal stream correlates with its source at -0.99), so the frame buffer that decodes to
// the source is the negated spectrum.  Sample 255 lands in frame-buffer word 256, which the transform overwrites before it
// reads: no target, value 0.
__device__ __forceinline__ int rd93Target(const float *frame, int k)
{
    const float r = roundf(frame[k] * -kRdK);
    return k == 255 ? 0 : static_cast<int>(fminf(fmaxf(r, -32768.0f), 32767.0f));
}

// DESIGN.md 10.11's quantiser with this R: the estimate (|t| * rcp) >> 24 with -1 .. +2 added, the smaller magnitude first,
// replaced on strictly less
__device__ __forceinline__ int rd93Nearest(int t, int scale, uint32_t rcp, int qmax, uint32_t m0)
{
    const int s = t > 0 ? 1 : t < 0 ? -1 : 0;
    const int est = static_cast<int>((static_cast<unsigned long long>(static_cast<uint32_t>(abs(t))) * rcp) >> 24);
    int best = 0, berr = 0;
#pragma unroll
    for (int d = -1 ; d <= 2 ; ++d)
    {
        const int q = min(max(s * (est + d), -qmax), qmax);
        const int err = abs(t - rd93Recon(q, scale, m0));
        if (d == -1 || err < berr) { best = q; berr = err; }
    }
    return best;
}

// the least w with -2^(w-1) <= v <= 2^(w-1) - 1
__device__ __forceinline__ int rd93Width(int v) { return 33 - __clz(v < 0 ? ~v : v); }
__device__ __forceinline__ int rd93Clamp(int q, int c) { return min(max(q, -(1 << c)), (1 << c) - 1); }     // to c + 1 bits
__device__ __forceinline__ int rd93Sub(int s) { return s < 16 ? 0 : s == kRd93Delta ? 1 : 2; }
__device__ __forceinline__ bool rd93Code0(int s) { return s == 0 || s == kRd93Hold; }
__device__ __forceinline__ int rd93Bits(int c) { return c == 0 ? 5 : 21 + 16 * c; }          // the proxy's: 5 bits of code, c + 1 a value

// what state s of a band leaves behind: the last value and the last difference, as the decoder keeps them (16 bits, signed)
__device__ __forceinline__ void rd93Out(int s, const Enc93RdRec &r, int *P, int *Dl)
{
    const int c = (s >= 1 && s <= 15) ? s : 15;
    const int a = rd93Clamp(r.q15, c), b = rd93Clamp(r.q14, c);
    *P = rd93Code0(s) ? 0 : a;
    *Dl = rd93Code0(s) ? 0 : static_cast<int16_t>(a - b);
}

// the width of the delta (s == 16) or double-delta (s == 17) option behind a predecessor that left (P, Dl); above 16: none
__device__ __forceinline__ int rd93DeltaWidth(int s, const Enc93RdRec &r, int P, int Dl)
{
    const int w1 = max(rd93Width(r.q0 - P), static_cast<int>(r.l1));
    const int w2 = max(max(rd93Width(r.q0 - P - Dl), rd93Width(r.q1 - 2 * r.q0 + P)), static_cast<int>(r.l2));
    return max(s == kRd93Delta ? w1 : w2, 2);
}

// the bits the decoder reads for a band in state s behind state p: the reuse bit where p's code was 0 (set: the whole
// band), 5 bits of code with the sub-type kept and 6 with it changed, sixteen values.  -1: no such step.  first: band 0,
// whose one predecessor is the frame's start state, standing in as the double-delta state with (P, Dl) = (0, 0)
__device__ __forceinline__ int rd93StepBits(int s, int p, const Enc93RdRec &r, int P, int Dl, bool first)
{
    const bool same = rd93Sub(p) == rd93Sub(s);
    const int head = (rd93Code0(p) ? 1 : 0) + (same ? 5 : 6);
    if (rd93Code0(s))
    {
        if (s == kRd93Hold && !(p == kRd93Hold || (first && p == kRd93DDelta)))
            return -1;
        return rd93Code0(p) && same ? 1 : head;
    }
    if (s < 16)
        return head + 16 * (s + 1);
    const int w = rd93DeltaWidth(s, r, P, Dl);
    return w <= 16 ? head + 16 * w : -1;
}

// S1: a block per stream-frame
__global__ __launch_bounds__(256) void enc93RdItemKernel(const EncTabs *__restrict__ Tp, const EncRdTabs *__restrict__ Rp, uint32_t m0,
    const float *__restrict__ spec, const uint32_t *__restrict__ frameStream, unsigned long long *__restrict__ items,
    Enc93RdRec *__restrict__ recs, unsigned long long *__restrict__ d0tot)
{
    __shared__ int st[256];
    __shared__ int16_t sq[256 * 64];
    __shared__ int sScale[64], sQmax[64];
    __shared__ uint32_t sRcp[64];
    const int tid = threadIdx.x;
    const uint32_t f = blockIdx.x;
    st[tid] = rd93Target(spec + static_cast<size_t>(f) * 256, tid);
    if (tid < 64) { sScale[tid] = Tp->scale[tid]; sQmax[tid] = Rp->qmax[tid]; sRcp[tid] = Rp->rcp[tid]; }
    __syncthreads();
    for (int i = tid ; i < 256 * 64 ; i += 256)
    {
        const int e = i & 63;
        sq[i] = static_cast<int16_t>(rd93Nearest(st[i >> 6], sScale[e], sRcp[e], sQmax[e], m0));
    }
    __syncthreads();
    unsigned long long *out = items + static_cast<size_t>(f) * kRd93ItemsPerFrame;
    for (int i = tid ; i < static_cast<int>(kRd93ItemsPerFrame) ; i += 256)
    {
        const int b = i >> 10, e = (i >> 4) & 63, c = i & 15;
        const int scale = sScale[e];
        unsigned long long D = 0;
        for (int j = 0 ; j < 16 ; ++j)
        {
            const int t = st[16 * b + j];
            const int d = c == 0 ? t : t - rd93Recon(rd93Clamp(sq[(16 * b + j) * 64 + e], c), scale, m0);
            D += static_cast<unsigned long long>(static_cast<uint32_t>(d) * static_cast<uint32_t>(d));
        }
        out[i] = D;
        if (c == 0 && e == 0)
            atomicAdd(&d0tot[frameStream[f] * 16 + b], D);
    }
    for (int i = tid ; i < static_cast<int>(kRd93RecsPerFrame) ; i += 256)
    {
        const int b = i >> 6, e = i & 63;
        const int16_t *q = sq + (16 * b) * 64 + e;
        int l1 = 1, l2 = 1;
        for (int j = 1 ; j < 16 ; ++j)
            l1 = max(l1, rd93Width(q[j * 64] - q[(j - 1) * 64]));
        for (int j = 2 ; j < 16 ; ++j)
            l2 = max(l2, rd93Width(q[j * 64] - 2 * q[(j - 1) * 64] + q[(j - 2) * 64]));
        recs[static_cast<size_t>(f) * kRd93RecsPerFrame + i] = Enc93RdRec{ q[0], q[64], q[14 * 64], q[15 * 64], static_cast<uint8_t>(l1),
                                                                          static_cast<uint8_t>(l2), { 0, 0 } };
    }
}

// S2: grid (kRd93ProxyPerJob / 256, chunks of kRd93ChunkFrames job-frames of the group); a thread per (band, scale code,
// lambda) walks the chunk's frames and adds what it summed to its job's row whenever the job changes and at the end
__global__ __launch_bounds__(256) void enc93RdProxyKernel(const EncRdTabs *__restrict__ Rp, const unsigned long long *__restrict__ items,
    const unsigned long long *__restrict__ floorE, const uint32_t *__restrict__ frameJob, const EncJob *__restrict__ jobs, uint32_t JF,
    unsigned long long *__restrict__ proxyJ, uint32_t *__restrict__ proxyB)
{
    const uint32_t idx = blockIdx.x * 256 + threadIdx.x;        // (kRd93ProxyPerJob is a multiple of 256)
    const uint32_t be = idx / kRdKL, li = idx % kRdKL;
    const unsigned long long lam = Rp->ladder[li];
    const uint32_t jf0 = blockIdx.y * kRd93ChunkFrames, jf1 = min(jf0 + kRd93ChunkFrames, JF);
    uint32_t cur = frameJob[jf0];
    EncJob job = jobs[cur];
    unsigned long long eb = floorE[job.set], accJ = 0;
    uint32_t accB = 0;
    for (uint32_t jf = jf0 ; jf < jf1 ; ++jf)
    {
        const uint32_t ji = frameJob[jf];
        if (ji != cur)
        {
            atomicAdd(&proxyJ[static_cast<size_t>(cur) * kRd93ProxyPerJob + idx], accJ);
            atomicAdd(&proxyB[static_cast<size_t>(cur) * kRd93ProxyPerJob + idx], accB);
            cur = ji; job = jobs[ji]; eb = floorE[job.set]; accJ = 0; accB = 0;
        }
        const unsigned long long *p = items + static_cast<size_t>(encSpecFrame(job, jf)) * kRd93ItemsPerFrame + be * 16;
        unsigned long long best = kRdInf;
        uint32_t bb = 0;
#pragma unroll
        for (int c = 0 ; c < 16 ; ++c)
        {
            const unsigned long long D = p[c];
            const unsigned long long cost = (D > eb ? D : eb) + lam * static_cast<unsigned long long>(rd93Bits(c));
            if (cost < best) { best = cost; bb = static_cast<uint32_t>(rd93Bits(c)); }        // (a tie: the lower option, fewer bits)
        }
        accJ += best; accB += bb;
    }
    atomicAdd(&proxyJ[static_cast<size_t>(cur) * kRd93ProxyPerJob + idx], accJ);
    atomicAdd(&proxyB[static_cast<size_t>(cur) * kRd93ProxyPerJob + idx], accB);
}

// S3: a block per job of the group, a thread per lambda: each band's scale code (least sum, then fewer bits, then the lower
// code) and the band count minimising the kept bands' sums plus the cut bands' energies (a tie to the smaller count)
__global__ __launch_bounds__(64) void enc93RdHeaderKernel(const unsigned long long *__restrict__ proxyJ, const uint32_t *__restrict__ proxyB,
    const unsigned long long *__restrict__ d0tot, const EncJob *__restrict__ jobs, Enc93RdHead *__restrict__ head)
{
    __shared__ unsigned long long sSuf[17];
    const uint32_t ji = blockIdx.x;
    const int li = threadIdx.x;
    const EncJob job = jobs[ji];
    if (li == 0)
    {
        sSuf[16] = 0;
        for (int b = 15 ; b >= 0 ; --b)
            sSuf[b] = sSuf[b + 1] + d0tot[job.stream * 16 + b];
    }
    __syncthreads();
    if (li >= kRdKL)
        return;
    Enc93RdHead h;
    unsigned long long pre = 0, bestTot = 0;
    int bn = 0;
    for (int b = 0 ; b < 16 ; ++b)
    {
        const size_t at = (static_cast<size_t>(ji) * 1024 + b * 64) * kRdKL + li;
        unsigned long long bJ = proxyJ[at];
        uint32_t bB = proxyB[at];
        int be = 0;
        for (int e = 1 ; e < 64 ; ++e)
        {
            const unsigned long long J = proxyJ[at + static_cast<size_t>(e) * kRdKL];
            const uint32_t B = proxyB[at + static_cast<size_t>(e) * kRdKL];
            if (J < bJ || (J == bJ && B < bB)) { bJ = J; bB = B; be = e; }
        }
        h.hv[b] = static_cast<uint8_t>(be);
        pre += bJ;
        const unsigned long long tot = pre + sSuf[b + 1];
        if (bn == 0 || tot < bestTot) { bestTot = tot; bn = b + 1; }
    }
    h.numBands = bn;
    head[ji * kRdKL + li] = h;
}

// S4 (PATH = false): grid (chunks of kRd93ChunkFrames job-frames, lambda); S6 (PATH = true): grid (chunks), the job's chosen
// lambda and header vector.  A block is eight 32-lane groups; group g takes job-frames g, g + 8, ... of the chunk.  Lane s
// of a group is state s of the band at hand (lanes 19..31 idle along); the cross-lane reads stay inside the group, whose
// lanes run the same bands together.
template <bool PATH>
__global__ __launch_bounds__(256) void enc93RdTrellisKernel(const EncRdTabs *__restrict__ Rp, const unsigned long long *__restrict__ items,
    const Enc93RdRec *__restrict__ recs, const unsigned long long *__restrict__ floorE, const uint32_t *__restrict__ frameJob,
    const EncJob *__restrict__ jobs, uint32_t JF, const Enc93RdHead *__restrict__ head, const Enc93RdChoice *__restrict__ choice,
    Enc93RdTot *__restrict__ tot, uint8_t *__restrict__ codes, uint32_t *__restrict__ frameBits)
{
    const int s = threadIdx.x & 31, g = threadIdx.x >> 5;
    const uint32_t jf0 = blockIdx.x * kRd93ChunkFrames, jf1 = min(jf0 + kRd93ChunkFrames, JF);
    const bool state = s < kRd93States;
    const int c = (s >= 1 && s <= 15) ? s : (s == 0 || s == kRd93Hold) ? 0 : 15;       // the state's item
    uint32_t cur = ~0u;
    unsigned long long accD = 0, accB = 0;
    for (uint32_t jf = jf0 + g ; jf < jf1 ; jf += 8)
    {
        const uint32_t ji = frameJob[jf];
        const EncJob job = jobs[ji];
        if (!PATH && s == 0 && ji != cur)
        {
            if (cur != ~0u)
            {
                atomicAdd(&tot[cur * kRdKL + blockIdx.y].D, accD);
                atomicAdd(&tot[cur * kRdKL + blockIdx.y].bits, accB);
            }
            cur = ji; accD = 0; accB = 0;
        }
        const int li = PATH ? choice[ji].ladderIndex : static_cast<int>(blockIdx.y);
        const int n = PATH ? choice[ji].numBands : head[ji * kRdKL + li].numBands;
        const uint8_t *hv = PATH ? choice[ji].hv : head[ji * kRdKL + li].hv;
        const unsigned long long lam = Rp->ladder[li], eb = floorE[job.set];
        const size_t sf = encSpecFrame(job, jf);
        unsigned long long V = s == kRd93DDelta ? 0 : kRdInf, TD = 0, survLo = 0, survHi = 0;
        uint32_t TB = 0;
        int P = 0, Dl = 0;
        for (int b = 0 ; b < n ; ++b)
        {
            const int e = hv[b];
            const Enc93RdRec r = recs[sf * kRd93RecsPerFrame + b * 64 + e];
            const unsigned long long D = items[sf * kRd93ItemsPerFrame + (b * 64 + e) * 16 + c];
            const unsigned long long md = D > eb ? D : eb;
            unsigned long long best = kRdInf;
            uint32_t bestB = 0;
            int bp = 0;
#pragma unroll
            for (int p = 0 ; p < kRd93States ; ++p)
            {
                const unsigned long long Vp = __shfl(V, p, 32);
                const uint32_t TBp = __shfl(TB, p, 32);
                const int Pp = __shfl(P, p, 32), Dlp = __shfl(Dl, p, 32);
                const int bits = rd93StepBits(s, p, r, Pp, Dlp, b == 0);
                const unsigned long long cost = Vp + md + lam * static_cast<unsigned long long>(static_cast<uint32_t>(max(bits, 0)));
                const uint32_t nb = TBp + static_cast<uint32_t>(max(bits, 0));
                // least cost, then fewer bits in all, then the lower predecessor
                if (state && bits >= 0 && Vp < kRdInf && (cost < best || (cost == best && nb < bestB))) { best = cost; bestB = nb; bp = p; }
            }
            const unsigned long long TDp = __shfl(TD, bp, 32);
            TD = best < kRdInf ? TDp + D : 0;
            TB = best < kRdInf ? bestB : 0;
            V = best;
            rd93Out(s, r, &P, &Dl);
            if (PATH)
            {
                if (b < 8) survLo |= static_cast<unsigned long long>(bp) << (5 * b);
                else survHi |= static_cast<unsigned long long>(bp) << (5 * (b - 8));
            }
        }
        // the end state: least cost, then fewer bits, then the lower state
        int ws = s;
        unsigned long long eV = V, eD = TD;
        uint32_t eB = TB;
#pragma unroll
        for (int off = 16 ; off >= 1 ; off >>= 1)
        {
            const unsigned long long oV = __shfl_xor(eV, off, 32), oD = __shfl_xor(eD, off, 32);
            const uint32_t oB = __shfl_xor(eB, off, 32);
            const int os = __shfl_xor(ws, off, 32);
            if (oV < eV || (oV == eV && (oB < eB || (oB == eB && os < ws)))) { eV = oV; eD = oD; eB = oB; ws = os; }
        }
        if (!PATH)
        {
            accD += eD; accB += eB;
            continue;
        }
        int at = ws;
        for (int b = 15 ; b >= 0 ; --b)
        {
            const unsigned long long word = b < 8 ? survLo : survHi;
            const int mine = static_cast<int>(word >> (5 * (b & 7))) & 31;
            const int before = __shfl(mine, at, 32);
            if (s == 0)
                codes[static_cast<size_t>(jf) * 16 + b] = static_cast<uint8_t>(b < n ? at : 0xFF);
            if (b < n)
                at = before;
        }
        if (s == 0)
            frameBits[jf] = eB;
    }
    if (!PATH && s == 0 && cur != ~0u)
    {
        atomicAdd(&tot[cur * kRdKL + blockIdx.y].D, accD);
        atomicAdd(&tot[cur * kRdKL + blockIdx.y].bits, accB);
    }
}

// S5: a thread per job of the group: over the 56 candidates the least D within the budget (ties: fewer bits, the lower
// ladder index), else the fewest bits (a tie: the lower ladder index)
__global__ __launch_bounds__(64) void enc93RdChooseKernel(const Enc93RdTot *__restrict__ tot, const Enc93RdHead *__restrict__ head,
    const unsigned long long *__restrict__ d0tot, const EncJob *__restrict__ jobs, const long long *__restrict__ budget, uint32_t n,
    Enc93RdChoice *__restrict__ choice)
{
    const uint32_t ji = blockIdx.x * 64 + threadIdx.x;
    if (ji >= n)
        return;
    const EncJob job = jobs[ji];
    const long long cap = budget[ji];
    int best = -1, least = -1;
    unsigned long long bestD = 0, bestB = 0, leastD = 0, leastB = 0;
    for (int li = 0 ; li < kRdKL ; ++li)
    {
        const Enc93RdTot t = tot[ji * kRdKL + li];
        unsigned long long D = t.D;
        for (int b = head[ji * kRdKL + li].numBands ; b < 16 ; ++b)
            D += d0tot[job.stream * 16 + b];
        if (least < 0 || t.bits < leastB) { least = li; leastD = D; leastB = t.bits; }
        if (cap >= 0 && t.bits <= static_cast<unsigned long long>(cap) && (best < 0 || D < bestD || (D == bestD && t.bits < bestB)))
        {
            best = li; bestD = D; bestB = t.bits;
        }
    }
    const int win = best >= 0 ? best : least;
    const Enc93RdHead h = head[ji * kRdKL + win];
    Enc93RdChoice ch = { win, h.numBands, best >= 0 ? 1 : 0, 0, best >= 0 ? bestB : leastB, best >= 0 ? bestD : leastD, {} };
    for (int b = 0 ; b < 16 ; ++b)
        ch.hv[b] = h.hv[b];
    choice[ji] = ch;
}

// the frame count and the sixteen header bytes of each job of the group; bands from numBands on are cut with 0xFF
__global__ __launch_bounds__(64) void enc93RdHeadKernel(const EncJob *__restrict__ jobs, const Enc93RdChoice *__restrict__ choice,
    const uint64_t *__restrict__ outOff, uint32_t n, uint32_t *__restrict__ W)
{
    const uint32_t si = blockIdx.x * 64 + threadIdx.x;
    if (si >= n)
        return;
    const Enc93RdChoice ch = choice[si];
    const uint64_t at = outOff[si] * 8;
    encPut(W, at, jobs[si].nFrames, 16);
    for (int b = 0 ; b < 16 ; ++b)
        encPut(W, at + 16 + 8 * b, b < ch.numBands ? static_cast<uint32_t>(ch.hv[b]) : 0xFFu, 8);
}

// S8: a block per job-frame, a lane per band: its bits, where they start, then the reuse bit, the code and the values
__global__ __launch_bounds__(64) void enc93RdPackKernel(const EncTabs *__restrict__ Tp, const EncRdTabs *__restrict__ Rp, uint32_t m0,
    const float *__restrict__ spec, const Enc93RdRec *__restrict__ recs, const uint32_t *__restrict__ frameJob,
    const EncJob *__restrict__ jobs, const Enc93RdChoice *__restrict__ choice, const uint8_t *__restrict__ codes,
    const uint32_t *__restrict__ frameOff, const uint64_t *__restrict__ outOff, uint32_t *__restrict__ W)
{
    __shared__ uint32_t sBits[16];
    const uint32_t jf = blockIdx.x, si = frameJob[jf];
    const int b = threadIdx.x;
    const EncJob job = jobs[si];
    const size_t sf = encSpecFrame(job, jf);
    const int n = choice[si].numBands;
    const bool live = b < n;
    int s = 0, p = kRd93DDelta, P = 0, Dl = 0, e = 0, bits = 0;
    Enc93RdRec r = {};
    if (live)
    {
        s = codes[static_cast<size_t>(jf) * 16 + b];
        e = choice[si].hv[b];
        r = recs[sf * kRd93RecsPerFrame + b * 64 + e];
        if (b > 0)
        {
            p = codes[static_cast<size_t>(jf) * 16 + b - 1];
            rd93Out(p, recs[sf * kRd93RecsPerFrame + (b - 1) * 64 + choice[si].hv[b - 1]], &P, &Dl);
        }
        bits = rd93StepBits(s, p, r, P, Dl, b == 0);
    }
    if (b < 16)
        sBits[b] = static_cast<uint32_t>(max(bits, 0));
    __syncthreads();
    if (!live || bits < 0)
        return;
    uint64_t pos = (outOff[si] + 18) * 8 + frameOff[jf];
    for (int j = 0 ; j < b ; ++j)
        pos += sBits[j];
    const bool same = rd93Sub(p) == rd93Sub(s);
    const bool reuse = rd93Code0(p) && rd93Code0(s) && same;
    if (rd93Code0(p))
    {
        encPut(W, pos, reuse ? 1u : 0u, 1);
        pos += 1;
    }
    if (reuse)
        return;
    const int w = rd93Code0(s) ? 0 : s < 16 ? s + 1 : rd93DeltaWidth(s, r, P, Dl);
    const uint32_t code = rd93Code0(s) ? 0u : static_cast<uint32_t>(w - 1);
    const uint32_t inc = rd93Sub(s) == (rd93Sub(p) + 1) % 3 ? 1u : 0u;
    encPut(W, pos, same ? code : (0x20u | inc << 4 | code), same ? 5 : 6);
    pos += same ? 5 : 6;
    if (w == 0)
        return;
    const int scale = Tp->scale[e], qmax = Rp->qmax[e], c = s < 16 ? s : 15;
    const uint32_t rcp = Rp->rcp[e], mask = 0xFFFFu >> (16 - w);
    const float *frame = spec + sf * 256;
    int q1 = P, q2 = P - Dl;                    // the values before this one: the predecessor's last two, as the decoder carries them
    for (int j = 0 ; j < 16 ; ++j)
    {
        const int q = rd93Clamp(rd93Nearest(rd93Target(frame, 16 * b + j), scale, rcp, qmax, m0), c);
        const int sym = s < 16 ? q : s == kRd93Delta ? q - q1 : q - 2 * q1 + q2;
        encPut(W, pos, static_cast<uint32_t>(sym) & mask, w);
        pos += static_cast<uint64_t>(w);
        q2 = q1; q1 = q;
    }
}

}  // namespace
