// dcs_encode_rd_fit.hip.h -- a set of streams encoded to ONE byte budget, included by dcs_encode.hip behind
// dcs_encode93_rd.hip.h, so that every other kernel keeps its place in the code object.
//
// dcs_encode_rd_streams and dcs_encode93_rd_streams hold each stream to a budget of its own.  Here the budgets are the
// result: every job's candidates (the totals R3 and S5 choose among) are kept as a curve of (size in bytes, squared error),
// one allocator run over all curves gives each job an allotment, and the per-stream choose kernels then run with the
// allotments as their budgets.  The allocation is exact integer arithmetic, stated once in DESIGN.md 10.13, restated in
// tests/encrd_fit_ref.py, and written twice here: fitAllotHost (dcs_encode_rd_allot with ctx NULL) and the kernels.
//
//   F1  encRdCurveKernel, enc93RdCurveKernel   a job's candidates from the group's totals into the call's curve table
//   F2  encFitHullKernel    a block of one wavefront per job: the cap, a rank sort by (size, D), then the staircase and its
//                           lower convex hull by one lane; the hull's vertices, the job's steps and its first allotment
//   F3  encFitSortKernel    all steps of all jobs by slope, compared by 128-bit cross-multiplication (FitStepBefore): a bitonic
//                           network over the step table padded to a power of two, one launch per compare-exchange distance
//   F4  encFitWalkKernel    one wavefront walks the ordered steps 64 at a time; then the fit record
//
// The walk is serial by definition (a step that does not fit stops its job for good, and the walk goes on).  F4 reaches the
// same result 64 steps at a time from two facts.  The remainder only falls, so a step larger than the remainder NOW is not
// taken at its turn either: it is either a miss or already behind one, and in both cases its job is stopped from its position
// on, which an atomic minimum on the job's stop position records in any order.  And among the steps that fit and are not
// behind a stop, the serial walk takes exactly the longest prefix whose sizes add up to at most the remainder; the step
// after that prefix is the next miss.

namespace {

constexpr uint32_t kFitMaxPoints = 3 * kRdKL;              // the most candidates a job has: three layouts of the R family
constexpr unsigned long long kFitAbsent = ~0ull;           // a slot of the curve table with no candidate (a layout not asked for)
constexpr unsigned long long kFitMaxD = 1ull << 62;        // accepted: D < 2^62 and sizes < 2^32 (the products need 94 bits)

// one hull edge of one job: taking it moves the job from the edge's first vertex to its second
struct FitStep { unsigned long long dD; uint32_t ds, job, index, sizeAfter; };     // ds 0: an unused slot, ordered last
static_assert(sizeof(FitStep) == 24, "FitStep");

// the order of the walk: dD / ds descending, exactly; ties by the lower job, then the earlier step
struct FitStepBefore
{
    __host__ __device__ bool operator()(const FitStep &a, const FitStep &b) const
    {
        if (a.ds == 0 || b.ds == 0)
            return a.ds != 0 && b.ds == 0;
        const unsigned __int128 l = static_cast<unsigned __int128>(a.dD) * b.ds, r = static_cast<unsigned __int128>(b.dD) * a.ds;
        if (l != r)
            return l > r;
        return a.job != b.job ? a.job < b.job : a.index < b.index;
    }
};

// the middle one of three staircase points stays on the hull when the slope into it is strictly steeper than the slope out
__host__ __device__ inline bool fitKeepsMiddle(unsigned long long sa, unsigned long long da, unsigned long long sb, unsigned long long db,
                                               unsigned long long sc, unsigned long long dc)
{
    return static_cast<unsigned __int128>(da - db) * (sc - sb) > static_cast<unsigned __int128>(db - dc) * (sb - sa);
}

// ------------------------------------------------------------------------------------------------ the allocator on the host

// Steps 1 to 3 for one job: `pts` (size, D) in the caller's order, absent slots skipped -> the hull's vertices.
void fitHullHost(const uint64_t *size, const uint64_t *D, uint64_t n, uint64_t cap, std::vector<std::pair<uint64_t, uint64_t>> &hull)
{
    std::vector<std::pair<uint64_t, uint64_t>> pts;
    uint64_t least = kFitAbsent, leastD = 0;
    for (uint64_t i = 0 ; i < n ; ++i)
    {
        if (size[i] == kFitAbsent)
            continue;
        if (size[i] < least) { least = size[i]; leastD = D[i]; }       // (the first of the smallest: what a pinned job keeps)
        if (size[i] <= cap)
            pts.emplace_back(size[i], D[i]);
    }
    hull.clear();
    if (pts.empty())
    {
        hull.emplace_back(least, leastD);
        return;
    }
    std::sort(pts.begin(), pts.end());
    uint64_t best = 0;
    for (size_t i = 0 ; i < pts.size() ; ++i)
    {
        if (i != 0 && pts[i].second >= best)
            continue;
        best = pts[i].second;
        while (hull.size() >= 2 && !fitKeepsMiddle(hull[hull.size() - 2].first, hull[hull.size() - 2].second, hull.back().first,
                                                   hull.back().second, pts[i].first, pts[i].second))
            hull.pop_back();
        hull.push_back(pts[i]);
    }
}

void fitAllotHost(const uint64_t *size, const uint64_t *D, const uint64_t *off, uint32_t nJobs, uint64_t total, const uint32_t *cap,
                  uint32_t *allot, DcsEncodeRdFitInfo *fit)
{
    std::vector<FitStep> steps;
    std::vector<std::pair<uint64_t, uint64_t>> hull;
    std::vector<uint64_t> errAt(nJobs);
    DcsEncodeRdFitInfo f{};
    f.totalBytes = total;
    for (uint32_t j = 0 ; j < nJobs ; ++j)
    {
        fitHullHost(size + off[j], D + off[j], off[j + 1] - off[j], cap != nullptr ? cap[j] : 0xFFFFFFFFull, hull);
        allot[j] = static_cast<uint32_t>(hull[0].first);
        errAt[j] = hull[0].second;
        f.leastBytes += hull[0].first;
        for (size_t i = 1 ; i < hull.size() ; ++i)
            steps.push_back(FitStep{ hull[i - 1].second - hull[i].second, static_cast<uint32_t>(hull[i].first - hull[i - 1].first), j,
                                     static_cast<uint32_t>(i - 1), static_cast<uint32_t>(hull[i].first) });
    }
    f.nSteps = static_cast<uint32_t>(steps.size());
    f.fits = f.leastBytes <= total ? 1 : 0;
    if (f.fits)
    {
        std::sort(steps.begin(), steps.end(), FitStepBefore());
        std::vector<uint8_t> stopped(nJobs, 0);
        uint64_t remaining = total - f.leastBytes;
        for (const FitStep &s : steps)
        {
            if (stopped[s.job])
                continue;
            if (s.ds > remaining)
            {
                stopped[s.job] = 1;
                continue;
            }
            remaining -= s.ds;
            allot[s.job] = s.sizeAfter;
            errAt[s.job] -= s.dD;
            ++f.stepsTaken;
        }
    }
    for (uint32_t j = 0 ; j < nJobs ; ++j)
    {
        f.usedBytes += allot[j];
        f.sqErr += errAt[j];
    }
    *fit = f;
}

// ----------------------------------------------------------------------------------------------------------- the kernels

// F1, the R family: a block per job of the group, a thread per (layout, lambda), the totals as R3 forms them; the slot of a
// layout the job's set does not ask for is absent.  (sizes in bytes: 18 + ceil(bits / 8))
__global__ __launch_bounds__(256) void encRdCurveKernel(const EncRdTot *__restrict__ tot, const unsigned long long *__restrict__ d0tot,
    const EncJob *__restrict__ jobs, const EncSet *__restrict__ sets, unsigned long long *__restrict__ curveSize,
    unsigned long long *__restrict__ curveD)
{
    __shared__ unsigned long long sSuf[17];
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
    if (tid >= 3 * kRdKL)
        return;
    const int v = tid / kRdKL, li = tid % kRdKL;
    const int nmin = v == 1 ? 3 : 1;
    unsigned long long preJ = 0, preD = 0, preB = 0, bestTot = 0, bD = 0, bBits = 0;
    int bn = 0;
    const bool asked = (set.vmask >> v) & 1u;
    if (asked)
        for (int b = 0 ; b < 16 ; ++b)
        {
            const EncRdTot *tb = tot + (((static_cast<size_t>(ji) * 3 + v) * 16 + b) * kRdNH) * kRdKL + li;
            EncRdTot bt = tb[static_cast<size_t>(kRdNH - 1) * kRdKL];
            for (int k = kRdNH - 2 ; k >= 0 ; --k)
            {
                const EncRdTot t = tb[static_cast<size_t>(k) * kRdKL];
                if (t.J < bt.J || (t.J == bt.J && t.bits < bt.bits)) bt = t;
            }
            preJ += bt.J; preD += bt.D; preB += bt.bits;
            const int n = b + 1;
            const unsigned long long totJ = preJ + sSuf[n];
            if (n >= nmin && (bn == 0 || totJ < bestTot)) { bestTot = totJ; bn = n; bD = preD + sSuf[n]; bBits = preB; }
        }
    const size_t at = static_cast<size_t>(ji) * kFitMaxPoints + tid;
    curveSize[at] = asked ? 18 + (bBits + 7) / 8 : kFitAbsent;
    curveD[at] = bD;
}

// F1, the S family: a thread per (job of the group, lambda), the totals as S5 forms them; the slots behind the 56 are absent
__global__ __launch_bounds__(64) void enc93RdCurveKernel(const Enc93RdTot *__restrict__ tot, const Enc93RdHead *__restrict__ head,
    const unsigned long long *__restrict__ d0tot, const EncJob *__restrict__ jobs, uint32_t n, unsigned long long *__restrict__ curveSize,
    unsigned long long *__restrict__ curveD)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x, ji = i / kFitMaxPoints, li = i % kFitMaxPoints;
    if (ji >= n)
        return;
    unsigned long long size = kFitAbsent, D = 0;
    if (li < static_cast<uint32_t>(kRdKL))
    {
        const Enc93RdTot t = tot[ji * kRdKL + li];
        D = t.D;
        for (int b = head[ji * kRdKL + li].numBands ; b < 16 ; ++b)
            D += d0tot[jobs[ji].stream * 16 + b];
        size = 18 + (t.bits + 7) / 8;
    }
    curveSize[i] = size;
    curveD[i] = D;
}

// F2: steps 1 to 3 for job blockIdx.x.  Its steps go to the slots of its points (off[j] ..), the unused ones with ds 0.
__global__ __launch_bounds__(64) void encFitHullKernel(const unsigned long long *__restrict__ size, const unsigned long long *__restrict__ D,
    const unsigned long long *__restrict__ off, const uint32_t *__restrict__ cap, FitStep *__restrict__ steps, uint32_t *__restrict__ vertN,
    uint32_t *__restrict__ vertSize, unsigned long long *__restrict__ vertD, uint32_t *__restrict__ allot, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long sS[kFitMaxPoints], sD[kFitMaxPoints], tS[kFitMaxPoints], tD[kFitMaxPoints];
    __shared__ uint32_t sCount, sHull;
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    const unsigned long long o0 = off[j];
    const uint32_t n = static_cast<uint32_t>(off[j + 1] - o0);          // (1 .. kFitMaxPoints: checked on the host)
    const unsigned long long c = cap != nullptr ? cap[j] : 0xFFFFFFFFull;
    if (lane == 0)
        sCount = 0;
    __syncthreads();
    // the points the cap leaves, the others pushed behind them (absent: size ~0)
    uint32_t kept = 0;
    for (uint32_t p = lane ; p < n ; p += 64)
    {
        const unsigned long long s = size[o0 + p];
        const bool in = s != kFitAbsent && s <= c;
        sS[p] = in ? s : kFitAbsent;
        sD[p] = D[o0 + p];
        kept += in ? 1u : 0u;
    }
    if (kept != 0)
        atomicAdd(&sCount, kept);
    __syncthreads();
    const uint32_t m = sCount;
    if (m == 0)
    {
        // pinned: the first of the smallest candidates alone
        if (lane == 0)
        {
            unsigned long long least = kFitAbsent, leastD = 0;
            for (uint32_t p = 0 ; p < n ; ++p)
            {
                const unsigned long long s = size[o0 + p];
                if (s < least) { least = s; leastD = D[o0 + p]; }
            }
            tS[0] = least; tD[0] = leastD;
            sHull = 1;
        }
    }
    else
    {
        // rank sort by (size, D, index)
        for (uint32_t p = lane ; p < n ; p += 64)
        {
            const unsigned long long s = sS[p], d = sD[p];
            uint32_t rank = 0;
            for (uint32_t q = 0 ; q < n ; ++q)
            {
                const unsigned long long s2 = sS[q], d2 = sD[q];
                rank += (s2 < s || (s2 == s && (d2 < d || (d2 == d && q < p)))) ? 1u : 0u;
            }
            tS[rank] = s; tD[rank] = d;
        }
        __syncthreads();
        // the staircase (a point stays when its D is strictly below every D before it) and its hull, in place in sS, sD
        if (lane == 0)
        {
            uint32_t h = 0;
            unsigned long long best = 0;
            for (uint32_t i = 0 ; i < m ; ++i)
            {
                const unsigned long long s = tS[i], d = tD[i];
                if (i != 0 && d >= best)
                    continue;
                best = d;
                while (h >= 2 && !fitKeepsMiddle(sS[h - 2], sD[h - 2], sS[h - 1], sD[h - 1], s, d))
                    --h;
                sS[h] = s; sD[h] = d;
                ++h;
            }
            sHull = h;
        }
        __syncthreads();
        for (uint32_t i = lane ; i < sHull ; i += 64) { tS[i] = sS[i]; tD[i] = sD[i]; }
    }
    __syncthreads();
    const uint32_t h = sHull;
    for (uint32_t i = lane ; i < n ; i += 64)
    {
        FitStep st{ 0, 0, j, 0, 0 };
        if (i >= 1 && i < h)
            st = FitStep{ tD[i - 1] - tD[i], static_cast<uint32_t>(tS[i] - tS[i - 1]), j, i - 1, static_cast<uint32_t>(tS[i]) };
        steps[o0 + i] = st;
        if (i < h) { vertSize[o0 + i] = static_cast<uint32_t>(tS[i]); vertD[o0 + i] = tD[i]; }
    }
    if (lane == 0)
    {
        vertN[j] = h;
        allot[j] = static_cast<uint32_t>(tS[0]);
        atomicAdd(&acc[0], tS[0]);
        atomicAdd(&acc[1], static_cast<unsigned long long>(h - 1));
    }
}

// F3: one compare-exchange pass of the bitonic network over n = 2^m steps: partners i and i ^ j, ascending (FitStepBefore)
// where i & k is 0.  Unused slots are equal to one another, which a sorting network does not mind.
__global__ __launch_bounds__(256) void encFitSortKernel(FitStep *__restrict__ steps, uint32_t n, uint32_t k, uint32_t j)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, l = i ^ j;
    if (i >= n || l <= i)
        return;
    const FitStep x = steps[i], y = steps[l];
    if ((i & k) == 0 ? FitStepBefore()(y, x) : FitStepBefore()(x, y))
    {
        steps[i] = y;
        steps[l] = x;
    }
}

// F4: one wavefront.  acc[0] = the base, acc[1] = the steps, which the sort has put before the unused slots.
__global__ __launch_bounds__(64) void encFitWalkKernel(const FitStep *__restrict__ steps, const unsigned long long *__restrict__ acc,
    const unsigned long long *__restrict__ off, const uint32_t *__restrict__ vertN, const uint32_t *__restrict__ vertSize,
    const unsigned long long *__restrict__ vertD, uint32_t nJobs, unsigned long long total, uint32_t *stopAt, uint32_t *allot,
    DcsEncodeRdFitInfo *__restrict__ fit)
{
    const uint32_t lane = threadIdx.x;
    const unsigned long long base = acc[0];
    const uint32_t S = static_cast<uint32_t>(acc[1]);
    const bool fits = base <= total;
    unsigned long long rem = fits ? total - base : 0;
    uint32_t taken = 0;
    for (uint32_t p0 = 0 ; p0 < S && rem > 0 ; p0 += 64)
    {
        const uint32_t pos = p0 + lane;
        bool open = pos < S;
        const FitStep st = open ? steps[pos] : FitStep{ 0, 0, 0, 0, 0 };
        for (;;)
        {
            // (the lanes of a wavefront are threads of their own to the compiler, which is free to let the lanes that read
            // below run before the lanes that record a stop here: the barrier orders them, the fence and the agent-scope
            // load carry the stop through the L2)
            if (open && st.ds > rem)
            {
                atomicMin(&stopAt[st.job], pos);
                open = false;
            }
            __threadfence();
            __syncthreads();
            if (open && __hip_atomic_load(&stopAt[st.job], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < pos)
                open = false;
            if (__ballot(open) == 0)
                break;
            unsigned long long sum = open ? st.ds : 0;
            for (int d = 1 ; d < 64 ; d <<= 1)
            {
                const unsigned long long o = __shfl_up(sum, d, 64);
                sum += static_cast<int>(lane) >= d ? o : 0;
            }
            const unsigned long long miss = __ballot(open && sum > rem);
            const int firstMiss = miss != 0 ? __ffsll(static_cast<long long>(miss)) - 1 : 64;
            const bool take = open && static_cast<int>(lane) < firstMiss;
            const unsigned long long takes = __ballot(take);
            if (take)
            {
                atomicMax(&allot[st.job], st.sizeAfter);
                open = false;
            }
            if (takes != 0)
            {
                rem -= __shfl(sum, 63 - __clzll(static_cast<long long>(takes)), 64);
                taken += static_cast<uint32_t>(__popcll(takes));
            }
            if (miss == 0)
                break;
        }
    }
    __threadfence();
    __syncthreads();
    // the record: the allotments and the error at each job's vertex of that size
    unsigned long long used = 0, err = 0;
    for (uint32_t j = lane ; j < nJobs ; j += 64)
    {
        const uint32_t a = __hip_atomic_load(&allot[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long o0 = off[j];
        used += a;
        for (uint32_t i = 0 ; i < vertN[j] ; ++i)
            if (vertSize[o0 + i] == a)
                err += vertD[o0 + i];
    }
    for (int d = 32 ; d >= 1 ; d >>= 1)
    {
        used += __shfl_xor(used, d, 64);
        err += __shfl_xor(err, d, 64);
    }
    if (lane == 0)
    {
        DcsEncodeRdFitInfo f{};
        f.totalBytes = total; f.leastBytes = base; f.usedBytes = used; f.sqErr = err;
        f.nSteps = S; f.stepsTaken = taken; f.fits = fits ? 1 : 0;
        *fit = f;
    }
}

// F2 to F4 queued on the arena's stream: curves of nJobs jobs (job j = points [off[j], off[j + 1]) of dSize, dD; N points in
// all, 1 .. kFitMaxPoints a job) -> dAllot[nJobs] and *dFit.  The buffers it needs are the arena's.
DcsStatus fitAllotDevice(DcsCtx *ctx, CacheArena &arena, const unsigned long long *dSize, const unsigned long long *dD,
                         const unsigned long long *dOff, uint32_t nJobs, size_t N, uint64_t total, const uint32_t *dCap, uint32_t *dAllot,
                         DcsEncodeRdFitInfo *dFit)
{
    const hipStream_t st = arena.stream();
    FitStep *dSteps;
    uint32_t *dVertN, *dVertSize, *dStop;
    unsigned long long *dVertD, *dAcc;
    if (N > 0x40000000u)                         // (positions in the ordered step table are 32 bits)
    {
        dcsCtxSetError(ctx, "more than 2^30 candidates in one allocation");
        return DCS_ERR_INVALID_ARG;
    }
    size_t P = 1;
    while (P < N)
        P <<= 1;
    ENCCHK(arena.alloc(&dSteps, P));
    ENCCHK(arena.alloc(&dVertN, nJobs));
    ENCCHK(arena.alloc(&dVertSize, N));
    ENCCHK(arena.alloc(&dVertD, N));
    ENCCHK(arena.alloc(&dStop, nJobs));
    ENCCHK(arena.alloc(&dAcc, 2));
    ENCCHK(hipMemsetAsync(dAcc, 0, sizeof(unsigned long long) * 2, st));
    ENCCHK(hipMemsetAsync(dStop, 0xFF, sizeof(uint32_t) * nJobs, st));
    ENCCHK(hipMemsetAsync(dSteps + N, 0, sizeof(FitStep) * (P - N), st));         // (ds 0: unused slots)
    hipLaunchKernelGGL(encFitHullKernel, dim3(nJobs), dim3(64), 0, st, dSize, dD, dOff, dCap, dSteps, dVertN, dVertSize, dVertD, dAllot, dAcc);
    const uint32_t n = static_cast<uint32_t>(P);
    for (uint32_t k = 2 ; k <= n && k != 0 ; k <<= 1)
        for (uint32_t j = k >> 1 ; j > 0 ; j >>= 1)
            hipLaunchKernelGGL(encFitSortKernel, dim3((n + 255) / 256), dim3(256), 0, st, dSteps, n, k, j);
    hipLaunchKernelGGL(encFitWalkKernel, dim3(1), dim3(64), 0, st, dSteps, dAcc, dOff, dVertN, dVertSize, dVertD, nJobs,
                       static_cast<unsigned long long>(total), dStop, dAllot, dFit);
    ENCCHK(hipGetLastError());
    return DCS_OK;
}

}  // namespace
