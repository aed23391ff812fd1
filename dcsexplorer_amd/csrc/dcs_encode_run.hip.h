// dcs_encode_run.hip.h -- the encoder's host driver: what a call is made of (EncInput, EncJobs, EncOutput,
// EncSweep), the state a call's steps share (EncState), the interface of a family of jobs (EncFamily), the families O, E and
// A, and the driver itself (EncRun).  dcs_encode.hip includes it behind the kernels of O, E and A; the families R and S and
// the shared-budget fit are declared here and defined behind their kernels (dcs_encode_rd.hip.h, dcs_encode93_rd.hip.h,
// dcs_encode_rd_fit.hip.h).  No kernel is defined here.

namespace {

// The device code object holds its kernel templates in the order in which the source first names an instantiation, and the
// project keeps that order fixed.  This list names the instantiations that the families below launch, in the
// order the code object has them, before any launch: so the families' methods may stand wherever they read best.  The
// templates of the headers included further down (resampler, WAV, FLAC, then R's and S's trellises) follow by their own
// first launches.
[[maybe_unused]] const void *const kEncTemplateOrder[] = {
    reinterpret_cast<const void *>(&enc93WalkKernel<0>), reinterpret_cast<const void *>(&enc93WalkKernel<1>),
    reinterpret_cast<const void *>(&encAnalyseKernel<int16_t>), reinterpret_cast<const void *>(&encAnalyseKernel<float>),
    reinterpret_cast<const void *>(&enc93aFrameKernel<false>), reinterpret_cast<const void *>(&enc93aFrameKernel<true>) };

// Where the driver reads its samples: the caller's float PCM on the host (dcs_encode_streams, dcs_encode93_streams), a
// decode batch's int16 PCM and error words, resident on the device (dcs_transcode_streams, dcs_transcode.hip.h), or the
// resampler's float output, resident on the device (dcs_encode_streams_at, dcs_resample.hip.h)
struct EncInput
{
    const uint64_t *sampleOffsets = nullptr;    // stream i = samples [sampleOffsets[i], sampleOffsets[i + 1]) of the one that is set:
    uint32_t nStreams = 0;
    const float *hostPcm = nullptr;
    const float *devFloat = nullptr;
    const int16_t *devPcm = nullptr;        // sampleOffsets[i] a multiple of 240 ...
    const uint32_t *devErr = nullptr;       // ... and its frames' error words at sampleOffsets[i] / 240
    const uint32_t *label = nullptr;        // the number a message gives stream i (null: i)
    const float *bound = nullptr;           // the largest |x| stream i may hold (null: 1; dcs_encode_files, INTEGRATION rule 12)
    const uint32_t *devStreamErr = nullptr; // devFloat: per stream, the error words of the decode its floats came from, ORed
                                            // (null: none did; encJoinPcmKernel, dcs_encode_join.hip.h)
    const volatile uint32_t *planFlag = nullptr;    // a word the device writes before the PCM is final: not 0 = the PCM is not to be used
    bool unusable = false;                  // (out) planFlag was set: DCS_ERR_BAD_STREAM, and nothing was written
};

// the jobs of a call: job j = (stream list[j].stream, set list[j].paramSet), every set of the one encoder `os93` names.
// A set that asks for (0x9301, Type 1) puts its jobs into the A family (dcs_encode93a.hip.h); only dcs_encode93a_streams
// and dcs_encode93a_sweep let one in.
struct EncJobs
{
    const DcsEncodeParams *sets;
    uint32_t nSets;
    const DcsSweepJob *list;
    uint32_t n;
    bool os93;
    bool search = false;                    // every job is searched to a budget: the R family (1994+ sets) or the S family (OS93 Type 0 sets)
    const uint32_t *budgetBytes = nullptr;  // search: per job, the most bytes its stream may have (null: the sets' targetBitRate)
    const struct EncFit *fit = nullptr;     // search: the jobs share one budget (dcs_encode_rd_fit.hip.h); budgetBytes is then null
};

// what dcs_encode_rd_fit and dcs_encode93_rd_fit ask of the driver: all jobs' streams together at most totalBytes, job j at
// most capBytes[j] (null: no caps); *info (or null) takes the allocator's record
struct EncFit { uint64_t totalBytes; const uint32_t *capBytes; DcsEncodeRdFitInfo *info; };

// after the sizes are known: the host memory that takes the `total` bytes (stream i at outOffsets[i]), or null for DCS_ERR_CAPACITY
using EncPlace = std::function<uint8_t *(const uint64_t *outOffsets, uint64_t total)>;

// where a call's streams and what is known of them go
struct EncOutput
{
    uint8_t *out = nullptr;                 // the caller's buffer of outCap bytes, where `place` is not given
    size_t outCap = 0;
    uint64_t *outOffsets = nullptr;         // nJobs + 1
    DcsEncodeInfo *info = nullptr;          // nJobs, or null
    const EncPlace *place = nullptr;
    DcsEncode93aInfo *info93a = nullptr;    // nJobs, or null: the Type-1 candidate of a job of the A family, zeros of any other
    DcsEncodeRdInfo *infoRd = nullptr;      // nJobs, or null: what the R or the S family's search chose
};

// what dcs_encode_sweep asks of the driver beyond a list of jobs
struct EncSweep
{
    DcsSweepResult *results = nullptr;
    bool measure = false;
    bool sizesOnly = false;                 // out == NULL && outCap == 0: nothing is packed for the host
};

// most job-frames a group may hold (0: what the memory takes); dcs_encode_sweep_group_frames
std::atomic<uint64_t> gGroupFrames{ 0 };

const int kCandType[4] = { 0, 0, 1, 1 }, kCandSub[4] = { 0, 3, 0, 3 };     // candidates in CloseStream's order (0,0), (0,3), (1,0), (1,3)

#define HIPTRY(call)                                                                                 \
    do {                                                                                             \
        const hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                        \
            return e_;                                                                               \
    } while (0)
#define ENCTRY(call)                                                                                 \
    do {                                                                                             \
        const DcsStatus s_ = (call);                                                                 \
        if (s_ != DCS_OK)                                                                            \
            return s_;                                                                               \
    } while (0)

// a decode queued by dcsSweepDecodeStart, released (which waits for the stream) on every way out of its scope
struct SweepDecodeGuard
{
    DcsSweepDecode *d = nullptr;
    ~SweepDecodeGuard() { dcsSweepDecodeRelease(d); }
};

// ------------------------------------------------------------------------------------------- what a call's steps share

// The state of one call that the driver and the families both touch: a plain struct, which every family holds a reference
// to.  Three lifetimes of device memory: `call`, `group` (emptied when an allocation attempt fails) and `blob` (taken anew
// for every group).  What only one family reads is that family's own.
struct EncState
{
    EncState(DcsCtx *ctx, EncInput &in, const EncJobs &jobs, const EncOutput &to)
        : ctx(ctx), st(dcsCtxStream(ctx)), in(in), jobs(jobs), to(to), call(ctx), group(ctx), blob(ctx) {}

    // ---- fixed by the arguments
    DcsCtx *const ctx;
    const hipStream_t st;
    EncInput &in;
    const EncJobs jobs;
    const EncOutput to;
    std::vector<EncStream> hs;                  // (checkStreams)
    uint32_t F = 0;                             // frames of all streams
    std::vector<EncSet> hsets;                  // (buildSets)
    struct EncSearchFamily *searched = nullptr; // the family that searches the call's jobs to budgets, if one does (its select)

    // ---- device buffers of the call: valid from allocCall to the end
    struct CallBufs
    {
        EncTabs *dT;
        float *dPcm = nullptr;                  // the host's PCM uploaded (null where the input is on the device)
        EncStream *dStr;
        EncSet *dSets;
        uint32_t *dFS;                          // frame -> stream
        float *dSpec, *dPw, *dLo, *dHi;         // E1's output per frame
        uint32_t *dBad;                         // per stream: a sample E1 refused
        float *dSums;                           // E2's sums per stream
    } cb;
    CacheArena call;

    // ---- device buffers of a group, sized for the largest one: valid from allocGroups to the end, their CONTENT that of
    // the resident group (runGroup), dOutOff of the group packed last
    struct GroupBufs
    {
        EncJob *dJobs;
        uint32_t *dFJ;                          // job-frame -> job of the group
        uint8_t *dHdr;
        int32_t *dKeep, *dWin;
        uint64_t *dSize, *dOutOff;
        uint32_t *dFrameOff;
    } gb;
    CacheArena group;

    // ---- the groups, and what is known of every job once its group has run
    std::vector<uint32_t> groupFirst;           // group g = jobs [groupFirst[g], groupFirst[g + 1])
    uint64_t groupFrames = 0;                   // the largest group's job-frames ...
    uint32_t groupJobs = 0;                     // ... and the most jobs in a group
    std::vector<EncJob> hj;                     // the resident group's jobs
    std::vector<int32_t> win, keep;             // per job (runGroup)
    std::vector<uint64_t> size;

    // ---- the packed group: valid from packGroup to the next one
    CacheArena blob;
    uint32_t *dW = nullptr;                     // the blob, big-endian after the swap
};

// A family of jobs: one encoder's share of every step of the driver.  A hook is called only of a family the call has jobs of
// (select), in the order O or E, A, R or S; its default does nothing.  A family owns its device pointers of both lifetimes
// and its host vectors; of the call it sees EncState alone.
struct EncFamily
{
    explicit EncFamily(EncState &s) : s(s), ctx(s.ctx), st(s.st), in(s.in), jobs(s.jobs), to(s.to), cb(s.cb), gb(s.gb) {}
    // once, behind buildSets: has the call jobs of this family?  What the family keeps of the sets and the job list
    virtual bool select() = 0;
    virtual DcsStatus allocCall() { return DCS_OK; }
    // the first failure is returned, for allocGroups to judge
    virtual hipError_t allocGroup() { return hipSuccess; }
    // behind E1, in front of bad[]'s way to the host: what the family adds up of E1's output per stream
    virtual DcsStatus streamSums() { return DCS_OK; }
    // behind that: what the family computes once per stream or stream-frame
    virtual DcsStatus analyse() { return DCS_OK; }
    // the family's launches for the n jobs (JF job-frames) of a group from job j0, in the group's buffers; a family that
    // shares no call with another queues what it reads back here as well
    virtual DcsStatus runGroup(uint32_t j0, uint32_t n, uint32_t JF) = 0;
    // behind every family's launches: the copies to the host of a family that does share calls
    virtual DcsStatus fetchGroup(uint32_t j0, uint32_t n) { return DCS_OK; }
    // behind the group's wait: win, keep and size of the family's jobs among the n from job j0
    virtual void sizeJobs(uint32_t j0, uint32_t n) {}
    // header and pack of the family's jobs of the resident group into the blob
    virtual DcsStatus packGroup(uint32_t n, uint32_t JF) = 0;
    // job j's share of the third byte that a measured sweep tells the decoder of (0: not a job of the family, or no share)
    virtual uint32_t head(uint32_t j) const { return 0; }
    // the family's own record of job j (info93a, infoRd)
    virtual void writeInfo(uint32_t j) {}

protected:
    ~EncFamily() = default;
    EncState &s;
    DcsCtx *const ctx;
    const hipStream_t st;
    const EncInput &in;
    const EncJobs &jobs;
    const EncOutput &to;
    EncState::CallBufs &cb;
    EncState::GroupBufs &gb;
};

// ------------------------------------------------------------------------------- O and E, the reference-equal encoders

// What O and E share: E2 (the sums per stream, the header per job), the frames' bits of up to three layouts per job-frame,
// the sizes and the winner (encSizeKernel), the 16-byte header into the blob, and win, keep and size read back.  A job of
// another family in the same group (A, in a sweep) has no layout here, cmask 0: encSizeKernel leaves its win at -1, which
// the head and pack kernels pass over.
struct EncLayoutFamily : EncFamily
{
    using EncFamily::EncFamily;
    hipError_t allocGroup() override { return s.group.alloc(&dFrameBits, 3 * static_cast<size_t>(s.groupFrames)); }
    DcsStatus streamSums() override
    {
        hipLaunchKernelGGL(encStreamKernel, dim3(in.nStreams), dim3(64), 0, st, cb.dStr, cb.dPw, cb.dLo, cb.dHi, cb.dSums);
        return DCS_OK;
    }
    DcsStatus fetchGroup(uint32_t j0, uint32_t n) override
    {
        ENCCHK(hipMemcpyAsync(s.win.data() + j0, gb.dWin, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        ENCCHK(hipMemcpyAsync(s.keep.data() + j0, gb.dKeep, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        ENCCHK(hipMemcpyAsync(s.size.data() + j0, gb.dSize, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, st));
        return DCS_OK;
    }

protected:
    ~EncLayoutFamily() = default;
    // the layouts any set of a call of this encoder asks for: bit 0 Type 0, bit 1 (1, 0), bit 2 (1, 3)
    bool selectLayouts(bool os93)
    {
        for (uint32_t k = 0 ; k < jobs.nSets && !jobs.search && jobs.os93 == os93 ; ++k)
            layouts |= s.hsets[k].vmask;
        return layouts != 0;
    }
    // in front of the band stages: the frames' bits cleared, the header half of E2
    DcsStatus headers(uint32_t n, uint32_t JF)
    {
        ENCCHK(hipMemsetAsync(dFrameBits, 0, sizeof(uint32_t) * 3 * JF, st));
        hipLaunchKernelGGL(encHeaderKernel, dim3(n), dim3(64), 0, st, cb.dT, gb.dJobs, cb.dSets, cb.dSums, gb.dHdr, gb.dKeep);
        return DCS_OK;
    }
    void sizes(uint32_t n, uint32_t JF)
    {
        hipLaunchKernelGGL(encSizeKernel, dim3(n), dim3(256), 0, st, gb.dJobs, cb.dSets, JF, dFrameBits, gb.dWin, gb.dSize, gb.dFrameOff);
    }
    void heads(uint32_t n)
    {
        hipLaunchKernelGGL(encHeadKernel, dim3(n), dim3(64), 0, st, gb.dJobs, gb.dHdr, gb.dWin, gb.dOutOff, s.dW);
    }
    uint32_t layouts = 0;
    uint32_t *dFrameBits = nullptr;             // [layout][job-frame]
};

// O: OS93 (O3-O5)
struct Enc93Family final : EncLayoutFamily
{
    using EncLayoutFamily::EncLayoutFamily;
    bool select() override { return selectLayouts(true); }
    hipError_t allocGroup() override
    {
        const size_t JF = static_cast<size_t>(s.groupFrames);
        HIPTRY(EncLayoutFamily::allocGroup());
        HIPTRY(s.group.alloc(&dRec, 32 * JF));
        HIPTRY(s.group.alloc(&dBand, 32 * JF));
        return hipSuccess;
    }
    DcsStatus runGroup(uint32_t, uint32_t n, uint32_t JF) override
    {
        ENCTRY(headers(n, JF));
        hipLaunchKernelGGL(enc93SearchKernel, dim3((JF + 3) / 4), dim3(128), 0, st, cb.dT, cb.dSpec, gb.dFJ, gb.dJobs, cb.dSets, gb.dHdr,
                           gb.dKeep, JF, dRec);
        if (layouts & 1)
            hipLaunchKernelGGL(enc93WalkKernel<0>, dim3((JF + 63) / 64), dim3(64), 0, st, cb.dT, gb.dJobs, cb.dSets, gb.dFJ, gb.dKeep, JF, JF,
                               dRec, dBand, dFrameBits);
        if (layouts & 2)
            hipLaunchKernelGGL(enc93WalkKernel<1>, dim3((n + 63) / 64), dim3(64), 0, st, cb.dT, gb.dJobs, cb.dSets, gb.dFJ, gb.dKeep, JF, n,
                               dRec, dBand, dFrameBits);
        sizes(n, JF);
        return DCS_OK;
    }
    DcsStatus packGroup(uint32_t n, uint32_t JF) override
    {
        heads(n);
        hipLaunchKernelGGL(enc93PackKernel, dim3((JF + 3) / 4), dim3(64), 0, st, cb.dT, cb.dSpec, gb.dFJ, gb.dJobs, gb.dHdr, gb.dKeep, gb.dWin,
                           JF, dBand, gb.dFrameOff, gb.dOutOff, s.dW);
        return DCS_OK;
    }

private:
    Enc93Rec *dRec = nullptr;
    Enc93Band *dBand = nullptr;
};

// E: 1994+ (E3-E5)
struct Enc94Family final : EncLayoutFamily
{
    using EncLayoutFamily::EncLayoutFamily;
    bool select() override { return selectLayouts(false); }
    hipError_t allocGroup() override
    {
        const size_t JF = static_cast<size_t>(s.groupFrames);
        HIPTRY(EncLayoutFamily::allocGroup());
        HIPTRY(s.group.alloc(&dBest, 128 * JF));
        HIPTRY(s.group.alloc(&dCodes, 48 * JF));
        HIPTRY(s.group.alloc(&dHdrBits, 48 * JF));
        HIPTRY(s.group.alloc(&dSmpBits, 48 * JF));
        return hipSuccess;
    }
    DcsStatus runGroup(uint32_t, uint32_t n, uint32_t JF) override
    {
        ENCTRY(headers(n, JF));
        ENCCHK(hipMemsetAsync(dBest, 0, size_t(128) * JF, st));
        ENCCHK(hipMemsetAsync(dCodes, 0, size_t(48) * JF, st));
        hipLaunchKernelGGL(encSearchKernel, dim3(JF), dim3(128), 0, st, cb.dT, cb.dSpec, cb.dLo, cb.dHi, gb.dFJ, gb.dJobs, cb.dSets, gb.dHdr,
                           gb.dKeep, dBest);
        hipLaunchKernelGGL(encChainKernel, dim3(n), dim3(64), 0, st, cb.dT, gb.dJobs, cb.dSets, gb.dKeep, JF,
                           reinterpret_cast<const uint64_t *>(dBest), dCodes);
        hipLaunchKernelGGL(encBitsKernel, dim3(JF), dim3(64), 0, st, cb.dT, cb.dSpec, gb.dFJ, gb.dJobs, cb.dSets, gb.dHdr, gb.dKeep, JF,
                           dCodes, dHdrBits, dSmpBits, dFrameBits);
        sizes(n, JF);
        return DCS_OK;
    }
    DcsStatus packGroup(uint32_t n, uint32_t JF) override
    {
        heads(n);
        hipLaunchKernelGGL(encPackKernel, dim3((JF + 3) / 4), dim3(64), 0, st, cb.dT, cb.dSpec, gb.dFJ, gb.dJobs, gb.dHdr, gb.dKeep, gb.dWin,
                           JF, dCodes, dHdrBits, dSmpBits, gb.dFrameOff, gb.dOutOff, s.dW);
        return DCS_OK;
    }

private:
    uint8_t *dBest = nullptr, *dCodes = nullptr, *dHdrBits = nullptr;
    uint16_t *dSmpBits = nullptr;
};

// ------------------------------------------------------------------- A, OS93a Type 1 (kernels: dcs_encode93a.hip.h)

struct Enc93aFamily final : EncFamily
{
    using EncFamily::EncFamily;
    // the family's sets by their distinct maximumQuantizationError; per (q, stream) that a job names, its row of A1's totals
    bool select() override
    {
        setQ.assign(jobs.nSets, kA93None);
        for (uint32_t k = 0 ; k < jobs.nSets ; ++k)
            if (isType1Of93a(jobs.sets[k]))
            {
                const float q = jobs.sets[k].maximumQuantizationError;
                const size_t at = std::find(qs.begin(), qs.end(), q) - qs.begin();
                if (at == qs.size())
                    qs.push_back(q);
                setQ[k] = static_cast<uint32_t>(at);
            }
        rowOf.assign(qs.size() * in.nStreams, kA93None);
        for (uint32_t j = 0 ; j < jobs.n ; ++j)
            if (mine(jobs.list[j].paramSet))
            {
                uint32_t &row = rowOf[static_cast<size_t>(setQ[jobs.list[j].paramSet]) * in.nStreams + jobs.list[j].stream];
                if (row == kA93None)
                    row = nRows++;
            }
        choice.resize(jobs.n);
        return !qs.empty();
    }
    DcsStatus allocCall() override
    {
        ENCCHK(s.call.alloc(&dA, 1));
        ENCCHK(s.call.alloc(&dFloorE, 18 * qs.size()));
        ENCCHK(s.call.alloc(&dSetQ, jobs.nSets));
        ENCCHK(s.call.alloc(&dRowOf, rowOf.size()));
        ENCCHK(s.call.alloc(&dTot, size_t(kA93Cand) * nRows));
        return DCS_OK;
    }
    hipError_t allocGroup() override
    {
        HIPTRY(s.group.alloc(&dChoice, s.groupJobs));
        HIPTRY(s.group.alloc(&dRec, static_cast<size_t>(s.groupFrames)));
        return hipSuccess;
    }
    // A1: one search per stream-frame that a job of the family names; kA93QPerLaunch of the distinct q to a launch
    DcsStatus analyse() override
    {
        const uint32_t nQ = static_cast<uint32_t>(qs.size());
        floorE.resize(size_t(18) * nQ);
        for (uint32_t k = 0 ; k < nQ ; ++k)
            floorE93a(qs[k], floorE.data() + size_t(18) * k);
        ENCCHK(hipMemcpyAsync(dA, &encTabs93a(), sizeof(Enc93aTabs), hipMemcpyHostToDevice, st));
        ENCCHK(hipMemcpyAsync(dFloorE, floorE.data(), sizeof(unsigned long long) * floorE.size(), hipMemcpyHostToDevice, st));
        ENCCHK(hipMemcpyAsync(dSetQ, setQ.data(), sizeof(uint32_t) * jobs.nSets, hipMemcpyHostToDevice, st));
        ENCCHK(hipMemcpyAsync(dRowOf, rowOf.data(), sizeof(uint32_t) * rowOf.size(), hipMemcpyHostToDevice, st));
        ENCCHK(hipMemsetAsync(dTot, 0, sizeof(Enc93aTot) * kA93Cand * nRows, st));
        for (uint32_t q0 = 0 ; q0 < nQ ; q0 += kA93QPerLaunch)
            hipLaunchKernelGGL(enc93aFrameKernel<false>, dim3(s.F), dim3(256), 0, st, dA, dFloorE, cb.dSpec, cb.dFS, dRowOf,
                               in.nStreams, q0, std::min(kA93QPerLaunch, nQ - q0), dTot, static_cast<const EncJob *>(nullptr),
                               static_cast<const uint32_t *>(nullptr), static_cast<const Enc93aChoice *>(nullptr), static_cast<Enc93aRec *>(nullptr));
        return DCS_OK;
    }
    // A2
    DcsStatus runGroup(uint32_t, uint32_t n, uint32_t) override
    {
        hipLaunchKernelGGL(enc93aChooseKernel, dim3(n), dim3(256), 0, st, dTot, dRowOf, in.nStreams, gb.dJobs, cb.dSets, dSetQ, dChoice);
        return DCS_OK;
    }
    DcsStatus fetchGroup(uint32_t j0, uint32_t n) override
    {
        ENCCHK(hipMemcpyAsync(choice.data() + j0, dChoice, sizeof(Enc93aChoice) * n, hipMemcpyDeviceToHost, st));
        return DCS_OK;
    }
    // a Type-1 job: the candidate (1, 0) of CloseStream's list, its header's band count, 3 header bytes and the frames' bits
    void sizeJobs(uint32_t j0, uint32_t n) override
    {
        for (uint32_t k = 0 ; k < n ; ++k)
            if (mine(s.hj[k].set))
            {
                s.win[j0 + k] = 2;
                s.keep[j0 + k] = choice[j0 + k].numBands;
                s.size[j0 + k] = 3 + (choice[j0 + k].frameBits + 7) / 8;
            }
    }
    // each job-frame's choices (A3), the frames' offsets (A4), the 3-byte headers and the pack (A5)
    DcsStatus packGroup(uint32_t n, uint32_t JF) override
    {
        hipLaunchKernelGGL(enc93aFrameKernel<true>, dim3(JF), dim3(256), 0, st, dA, dFloorE, cb.dSpec, gb.dFJ,
                           static_cast<const uint32_t *>(nullptr), 0u, 0u, 0u, static_cast<Enc93aTot *>(nullptr), gb.dJobs, dSetQ,
                           dChoice, dRec);
        hipLaunchKernelGGL(enc93aOffsetKernel, dim3(n), dim3(256), 0, st, gb.dJobs, dSetQ, dRec, gb.dFrameOff);
        hipLaunchKernelGGL(enc93aHeadKernel, dim3((n + 63) / 64), dim3(64), 0, st, gb.dJobs, dSetQ, dChoice, gb.dOutOff, n, s.dW);
        hipLaunchKernelGGL(enc93aPackKernel, dim3(JF), dim3(128), 0, st, dA, cb.dSpec, gb.dFJ, gb.dJobs, dSetQ, dChoice,
                           dRec, gb.dFrameOff, gb.dOutOff, s.dW);
        return DCS_OK;
    }
    // 1 pp bbbbb
    uint32_t head(uint32_t j) const override
    {
        return mine(jobs.list[j].paramSet) ? 0x80u | static_cast<uint32_t>(choice[j].selector) << 5 | static_cast<uint32_t>(s.keep[j]) : 0u;
    }
    void writeInfo(uint32_t j) override
    {
        if (to.info93a == nullptr || !mine(jobs.list[j].paramSet))
            return;
        const DcsEncodeParams &p = jobs.sets[jobs.list[j].paramSet];
        const Enc93aChoice &c = choice[j];
        const uint64_t budget = static_cast<uint64_t>(p.targetBitRate) * static_cast<uint64_t>(s.hs[jobs.list[j].stream].nFrames) * 240ull / 31250ull;
        to.info93a[j] = DcsEncode93aInfo{ c.selector, c.ladderIndex, c.numBands, 0, c.frameBits, budget, c.sumD };
    }

private:
    bool mine(uint32_t set) const { return setQ[set] != kA93None; }
    // the distinct maximumQuantizationError values of the family's sets, each set's index among them (kA93None: a set of the
    // O family), and per (q, stream) that a job names its row of A1's totals (kA93None: none does)
    std::vector<float> qs;
    std::vector<uint32_t> setQ, rowOf;
    uint32_t nRows = 0;
    std::vector<unsigned long long> floorE;     // [q][18] (analyse; the source of an asynchronous upload)
    std::vector<Enc93aChoice> choice;           // per job (runGroup)
    Enc93aTabs *dA = nullptr;                   // ---- of the call (A1)
    unsigned long long *dFloorE = nullptr;      // [q][18]
    uint32_t *dSetQ = nullptr, *dRowOf = nullptr;
    Enc93aTot *dTot = nullptr;                  // [row][candidate]
    Enc93aChoice *dChoice = nullptr;            // ---- of the group (A2-A5)
    Enc93aRec *dRec = nullptr;
};

// ------------------------------------------------- R and S, the families searched to a budget

// What R and S share, and what the shared-budget fit asks of either: the jobs' budgets and their way to the device; the
// candidates of a group's jobs as curves; the choice made again with other budgets; a job's error.
struct EncSearchFamily : EncFamily
{
    using EncFamily::EncFamily;
    // F1 behind the totals of the resident group's n jobs: their candidates' sizes and errors, kFitMaxPoints slots a job
    virtual void launchCurves(uint32_t n, unsigned long long *dSize, unsigned long long *dD) = 0;
    // the choice of the resident group's n jobs (from job j0) again, with budgetRd as it now stands
    DcsStatus chooseAgain(uint32_t j0, uint32_t n)
    {
        ENCTRY(uploadBudgets(j0, n));
        launchChoose(n);
        return fetchChoice(j0, n);
    }
    virtual unsigned long long sumD(uint32_t j) const = 0;
    std::vector<long long> budgetRd;            // per job, in frame bits (-1: nothing fits)

protected:
    ~EncSearchFamily() = default;
    bool selectSearch(bool os93)
    {
        if (!jobs.search || jobs.os93 != os93)
            return false;
        s.searched = this;
        return true;
    }
    // the budgets of all jobs
    void budgets()
    {
        budgetRd.resize(jobs.n);
        for (uint32_t j = 0 ; j < jobs.n ; ++j)
        {
            const uint64_t nF = s.hs[jobs.list[j].stream].nFrames;
            if (jobs.budgetBytes == nullptr)
                budgetRd[j] = static_cast<long long>(static_cast<uint64_t>(jobs.sets[jobs.list[j].paramSet].targetBitRate) * nF * 240ull / 31250ull);
            else
                budgetRd[j] = jobs.budgetBytes[j] >= 18 ? (static_cast<long long>(jobs.budgetBytes[j]) - 18) * 8 : -1;
        }
    }
    DcsStatus uploadBudgets(uint32_t j0, uint32_t n)
    {
        ENCCHK(hipMemcpyAsync(dBudget, budgetRd.data() + j0, sizeof(long long) * n, hipMemcpyHostToDevice, st));
        return DCS_OK;
    }
    virtual void launchChoose(uint32_t n) = 0;
    virtual DcsStatus fetchChoice(uint32_t j0, uint32_t n) = 0;
    std::vector<unsigned long long> floorRd;    // E_b per set: [set][16] of R, [set] of S (every band has sixteen samples)
    long long *dBudget = nullptr;               // of the group: [job]
};

// R: 1994+ searched (R1-R6; defined behind the kernels, dcs_encode_rd.hip.h)
struct EncRdFamily final : EncSearchFamily
{
    using EncSearchFamily::EncSearchFamily;
    bool select() override;
    DcsStatus allocCall() override;
    hipError_t allocGroup() override;
    DcsStatus analyse() override;
    DcsStatus runGroup(uint32_t j0, uint32_t n, uint32_t JF) override;
    void sizeJobs(uint32_t j0, uint32_t n) override;
    DcsStatus packGroup(uint32_t n, uint32_t JF) override;
    void writeInfo(uint32_t j) override;
    void launchCurves(uint32_t n, unsigned long long *dSize, unsigned long long *dD) override;
    unsigned long long sumD(uint32_t j) const override { return choice[j].sumD; }

private:
    void launchChoose(uint32_t n) override;
    DcsStatus fetchChoice(uint32_t j0, uint32_t n) override;
    std::vector<EncRdChoice> choice;            // per job: what R3 chose
    EncRdTabs *dR = nullptr;                    // ---- of the call (R1)
    unsigned long long *dItems = nullptr;       // [stream-frame][band][width][scale code]
    uint32_t *dPeak = nullptr;                  // [stream][band]
    unsigned long long *dD0 = nullptr, *dFloor = nullptr;   // [stream][band], [set][band]
    EncRdTot *dTot = nullptr;                   // ---- of the group (R2-R6): [job][layout][band][window index][lambda]
    EncRdChoice *dChoice = nullptr;
    uint8_t *dSurv = nullptr, *dEnd = nullptr, *dCodes = nullptr;   // [job-frame][band][state], [job][band], [job-frame][band]
    uint32_t *dBits = nullptr;                  // [job-frame]
};

// S: OS93 Type 0 searched (S1-S8; defined behind the kernels, dcs_encode93_rd.hip.h)
struct Enc93RdFamily final : EncSearchFamily
{
    using EncSearchFamily::EncSearchFamily;
    bool select() override;
    DcsStatus allocCall() override;
    hipError_t allocGroup() override;
    DcsStatus analyse() override;
    DcsStatus runGroup(uint32_t j0, uint32_t n, uint32_t JF) override;
    void sizeJobs(uint32_t j0, uint32_t n) override;
    DcsStatus packGroup(uint32_t n, uint32_t JF) override;
    void writeInfo(uint32_t j) override;
    void launchCurves(uint32_t n, unsigned long long *dSize, unsigned long long *dD) override;
    unsigned long long sumD(uint32_t j) const override { return choice[j].sumD; }

private:
    void launchChoose(uint32_t n) override;
    DcsStatus fetchChoice(uint32_t j0, uint32_t n) override;
    std::vector<Enc93RdChoice> choice;          // per job: what S5 chose
    EncRdTabs *dR = nullptr;                    // ---- of the call (S1)
    unsigned long long *dItems = nullptr;       // [stream-frame][band][scale code][option]
    Enc93RdRec *dRecs = nullptr;                // [stream-frame][band][scale code]
    unsigned long long *dD0 = nullptr, *dFloor = nullptr;   // [stream][band], [set]
    unsigned long long *dProxyJ = nullptr;      // ---- of the group (S2-S8): [job][band][scale code][lambda]
    uint32_t *dProxyB = nullptr;
    Enc93RdHead *dHead = nullptr;               // [job][lambda]
    Enc93RdTot *dTot = nullptr;                 // [job][lambda]
    Enc93RdChoice *dChoice = nullptr;
    uint8_t *dCodes = nullptr;                  // [job-frame][band]: the band's state
    uint32_t *dBits = nullptr;                  // [job-frame]
};

// The shared-budget fit (F1-F4; defined behind its kernels, dcs_encode_rd_fit.hip.h): no family, a mode of a call whose
// jobs R or S searches (s.searched).  Every group leaves its jobs' candidates in the call's curve table (curves); the
// allocator runs over all jobs (allot), after which the allotments are the jobs' budgets and sizes; each group then chooses
// again before it is packed (rechoose where it is still resident, the driver's runGroup where it is not), and report
// checks the sizes.
struct EncFitRun
{
    explicit EncFitRun(EncState &s) : s(s), ctx(s.ctx), st(s.st), jobs(s.jobs) {}
    DcsStatus allocCall();
    void launchCurves(uint32_t j0, uint32_t n);
    DcsStatus allot();
    DcsStatus rechoose(uint32_t g);
    DcsStatus report(uint32_t j);
    void record();
    bool allotted = false;                      // allot has run: a group that runs now chooses with its allotments, and leaves no curves

private:
    EncState &s;
    DcsCtx *const ctx;
    const hipStream_t st;
    const EncJobs &jobs;
    std::vector<uint32_t> allotBytes;           // per job
    DcsEncodeRdFitInfo rec{};                   // the allocator's record
    unsigned long long *dCurveSize = nullptr, *dCurveD = nullptr;   // of the call: [job][kFitMaxPoints], every job's candidates
    unsigned long long *dOff = nullptr;         // [job + 1]
    uint32_t *dCap = nullptr, *dAllot = nullptr;
    DcsEncodeRdFitInfo *dFit = nullptr;
};

// ------------------------------------------------------------------------------------------------------------ the driver

// The one host driver behind every encode, as an object that lives for one call.  A job is (stream, parameter set);
// dcs_encode_streams and its kin are one job per stream with one set.  The driver owns the steps and what every job needs;
// what one encoder needs is a family's (EncFamily: O, E, A, R, S, each a member here), and a step reaches the families only
// by walking `fams`, the ones the call has jobs of.  run() strings the steps together, each a member function below, in
// this order:
//   checkStreams   the streams' lengths, before anything is written; then the empty call's zeros, before any HIP call
//   buildSets      the parameter sets as the kernels read them; then every family's select: `fams`
//   allocCall      the buffers that live as long as the call (CallBufs, and the families')
//   allocGroups    the jobs in groups, runs of the job list whose per-job-frame buffers (GroupBufs and the families', sized for
//                  the largest group) fit the memory: makeGroups + allocGroup, one group unless a cap is set or an allocation fails
//   analyse        upload and E1, once per stream; the families' streamSums (O, E: the sums of E2), bad[] sets out for the
//                  host, the families' analyse (A1, R1, S1)
//   runGroup       per group: the families' runGroup (O or E on the jobs whose set has a layout of theirs, A2 on the Type-1
//                  jobs, R2-R3, S2-S5) and fetchGroup, a wait, and the families' sizeJobs, after which win, keep and size of
//                  the group's jobs are on the host.  After the first group's wait, checkInput: planFlag, then bad[]
//   fit.allot      (a fit call only) once every group has run and left its jobs' candidates in the call's curve table: see
//                  EncFitRun.  A call of one group runs its trellises once
//   placeOutput    once every size is known: outOffsets, info, results, and the memory the bytes go to (the capacity check)
//   packGroup      per group again (one that is no longer resident is first computed again by runGroup): layout, the
//                  families' packGroup and the swap into the group's blob on the device; then one of
//   deliverGroup   the blob to its place in the output, or with sweep.measure
//   measureGroup   the group's streams decoded where the pack step left them and compared with their sources (M1), the
//                  blob staged on the host when the decode or the output needs it there (stageBlob)
// The destructor waits for the stream once and gives back the arenas blob, group, call, in that order.
class EncRun : EncState
{
public:
    EncRun(DcsCtx *ctx, EncInput &in, const EncJobs &jobs, const EncOutput &to, const EncSweep &sweep)
        : EncState(ctx, in, jobs, to), sweep(sweep), dev(in.devPcm != nullptr), devF(in.devFloat != nullptr),
          famO(*this), famE(*this), famA(*this), famR(*this), famS(*this), fit(*this) {}
    ~EncRun()
    {
        if (!call.empty())
            call.wait();
        blob.clear();
        group.clear();
        call.clear();
    }
    DcsStatus run();

private:
    DcsStatus checkStreams();
    void buildSets();
    DcsStatus allocCall();
    void makeGroups(uint64_t limit);
    hipError_t allocGroup();
    DcsStatus allocGroups();
    DcsStatus analyse();
    DcsStatus runGroup(uint32_t g);
    DcsStatus checkInput();
    void writeInfo(uint32_t j);
    DcsStatus placeOutput();
    DcsStatus layoutGroup(uint32_t g, size_t *nWords);
    DcsStatus packGroup(uint32_t g);
    DcsStatus deliverGroup(uint32_t g);
    DcsStatus stageBlob();
    void selectDecodes(uint32_t n);
    DcsStatus decodeAndCompare(uint32_t n, bool onHost, bool *unusable);
    DcsStatus reportGroup(uint32_t g);
    DcsStatus measureGroup(uint32_t g);
    std::string name(uint32_t i) const { return "stream " + std::to_string(in.label ? in.label[i] : i); }

    const EncSweep sweep;
    const bool dev, devF;                       // the input is a decode batch's int16 PCM / float PCM on the device
    Enc93Family famO;
    Enc94Family famE;
    Enc93aFamily famA;
    EncRdFamily famR;
    Enc93RdFamily famS;
    std::vector<EncFamily *> fams;              // (buildSets) the families the call has jobs of
    EncFitRun fit;
    const EncTabs *tabs = nullptr;              // (buildSets) the one encoder's tables
    std::vector<uint32_t> frameStream;          // (checkStreams)
    uint64_t allFrames = 0, largest = 0;        // job-frames of all jobs, of the largest job
    uint32_t resident = ~0u, residentFrames = 0;    // the group whose rows the group buffers hold, and its job-frames
    std::vector<uint32_t> frameJob;             // the resident group's rows
    std::vector<uint32_t> bad;                  // per stream, on the host after the first group's wait
    std::vector<uint32_t> decodeErr;            // in.devStreamErr beside it (empty: the input has none)
    uint8_t *dst = nullptr;                     // where the bytes go (placeOutput); null: nowhere

    // ---- the packed group: valid from packGroup to the next one
    size_t blobLen = 0;
    std::vector<uint64_t> offs;                 // job k of the group at blob byte offs[k]
    std::vector<DcsSweepStream> ss;             // (sweep.measure) what the decoder is told of each
    std::vector<uint8_t> stage;                 // the blob on the host ...
    bool staged = false;                        // ... once stageBlob has run for this group

    // ---- measureGroup's own (sweep.measure only, M1)
    EncMeasure *dMeas = nullptr;                // of the group
    uint32_t *dFirstDec = nullptr;
    std::vector<uint32_t> sel, firstDec;        // the jobs of the group that are decoded; per job its first decoded frame
    std::vector<DcsSweepStream> selS;
    std::vector<uint64_t> selOff;
    uint32_t mostFrames = 0;                    // of the selected jobs: the longest ...
    uint64_t selFrames = 0;                     // ... and all of them
    std::vector<EncMeasure> meas;
};

DcsStatus EncRun::checkStreams()
{
    hs.resize(in.nStreams);
    for (uint32_t i = 0 ; i < in.nStreams ; ++i)
    {
        const uint64_t *so = in.sampleOffsets;
        if (so[i + 1] <= so[i])
        {
            dcsCtxSetError(ctx, (name(i) + ": empty").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        const uint64_t n = so[i + 1] - so[i];
        const uint64_t nF = (n + 239) / 240;
        if (nF > 65535)
        {
            dcsCtxSetError(ctx, (name(i) + ": more than 65 535 frames").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        if (sweep.measure && nF == 65535)
        {
            dcsCtxSetError(ctx, (name(i) + ": 65 535 frames; measured with the extra frame its decode would need 65 536, more than the frame count holds").c_str());
            return DCS_ERR_INVALID_ARG;
        }
        hs[i] = EncStream{ so[i] - so[0], static_cast<uint32_t>(n), F, static_cast<uint32_t>(nF),
                           dev ? static_cast<uint32_t>(so[i] / 240) : 0u, in.bound != nullptr ? in.bound[i] : 1.0f };
        frameStream.insert(frameStream.end(), static_cast<size_t>(nF), i);
        F += static_cast<uint32_t>(nF);
    }
    return DCS_OK;
}

// the sets, the jobs' frames, and the one place that says which families a call has
void EncRun::buildSets()
{
    tabs = jobs.os93 ? &encTabs93() : &encTabs();
    hsets.resize(jobs.nSets);
    for (uint32_t k = 0 ; k < jobs.nSets ; ++k)
    {
        const DcsEncodeParams &p = jobs.sets[k];
        const int typ = p.streamFormatType, sub = jobs.os93 ? 0 : p.streamFormatSubType;
        uint32_t cmask = 0;
        for (int c = 0 ; c < 4 ; ++c)
            if ((typ < 0 || typ == kCandType[c]) && (sub < 0 || sub == kCandSub[c])
                && !(jobs.os93 && p.formatVersion == 0x9301 && kCandType[c] == 1))
                cmask |= 1u << c;
        // (a Type-1 set of the A family: cmask 0, no O stage touches its jobs)
        const uint32_t vmask = ((cmask & 3) ? 1u : 0u) | ((cmask & 4) ? 2u : 0u) | ((cmask & 8) ? 4u : 0u);
        hsets[k] = EncSet{ p.powerBandCutoff, p.minimumDynamicRange, p.maximumQuantizationError, p.targetBitRate, vmask, cmask };
    }
    for (uint32_t j = 0 ; j < jobs.n ; ++j)
    {
        const uint64_t nF = hs[jobs.list[j].stream].nFrames;
        allFrames += nF;
        largest = nF > largest ? nF : largest;
    }
    for (EncFamily *f : std::initializer_list<EncFamily *>{ &famO, &famE, &famA, &famR, &famS })
        if (f->select())
            fams.push_back(f);
}

DcsStatus EncRun::allocCall()
{
    const uint32_t nStreams = in.nStreams;
    ENCCHK(call.alloc(&cb.dT, 1));
    if (!dev && !devF)
        ENCCHK(call.alloc(&cb.dPcm, in.sampleOffsets[nStreams] - in.sampleOffsets[0]));
    ENCCHK(call.alloc(&cb.dStr, nStreams));
    ENCCHK(call.alloc(&cb.dSets, jobs.nSets));
    ENCCHK(call.alloc(&cb.dFS, F));
    ENCCHK(call.alloc(&cb.dSpec, size_t(256) * F));
    ENCCHK(call.alloc(&cb.dPw, size_t(16) * F));
    ENCCHK(call.alloc(&cb.dLo, size_t(16) * F));
    ENCCHK(call.alloc(&cb.dHi, size_t(16) * F));
    ENCCHK(call.alloc(&cb.dBad, nStreams));
    ENCCHK(call.alloc(&cb.dSums, size_t(48) * nStreams));
    for (EncFamily *f : fams)
        ENCTRY(f->allocCall());
    if (jobs.fit != nullptr)
        ENCTRY(fit.allocCall());
    return DCS_OK;
}

// the groups: runs of the job list of at most `limit` job-frames, a job never split
void EncRun::makeGroups(uint64_t limit)
{
    groupFirst.assign(1, 0);
    groupFrames = 0; groupJobs = 0;
    uint64_t inGroup = 0;
    for (uint32_t j = 0 ; j < jobs.n ; ++j)
    {
        const uint64_t nF = hs[jobs.list[j].stream].nFrames;
        if ((inGroup != 0 && inGroup + nF > limit) || inGroup + nF > 0xFFFFFFFFull)
        {
            groupFirst.push_back(j);
            inGroup = 0;
        }
        inGroup += nF;
        groupFrames = inGroup > groupFrames ? inGroup : groupFrames;
        groupJobs = std::max(groupJobs, j + 1 - groupFirst.back());
    }
    groupFirst.push_back(jobs.n);
}

// every buffer of a group, sized for the largest one; the first failure is returned, for allocGroups to judge
hipError_t EncRun::allocGroup()
{
    const size_t JF = static_cast<size_t>(groupFrames), NJ = groupJobs;
    HIPTRY(group.alloc(&gb.dJobs, NJ));
    HIPTRY(group.alloc(&gb.dFJ, JF));
    HIPTRY(group.alloc(&gb.dHdr, 48 * NJ));
    HIPTRY(group.alloc(&gb.dKeep, NJ));
    HIPTRY(group.alloc(&gb.dWin, NJ));
    HIPTRY(group.alloc(&gb.dSize, NJ));
    HIPTRY(group.alloc(&gb.dOutOff, NJ));
    HIPTRY(group.alloc(&gb.dFrameOff, JF));
    for (EncFamily *f : fams)
        HIPTRY(f->allocGroup());
    if (sweep.measure)
    {
        HIPTRY(group.alloc(&dMeas, NJ));
        HIPTRY(group.alloc(&dFirstDec, NJ));
    }
    return hipSuccess;
}

// all jobs in one group when that can be had (or the cap that is set); half the job-frames each time the memory runs out
DcsStatus EncRun::allocGroups()
{
    uint64_t limit = gGroupFrames.load() != 0 ? std::max<uint64_t>(gGroupFrames.load(), largest) : allFrames;
    for (;;)
    {
        makeGroups(limit);
        const hipError_t e = allocGroup();
        if (e == hipSuccess)
            return DCS_OK;
        group.clear();
        if (e != hipErrorOutOfMemory || groupFrames <= largest)
            ENCCHK(e);
        limit = std::max<uint64_t>(largest, groupFrames / 2);
    }
}

// Upload and E1, the families' sums per stream; bad[] is on its way to the host, there after the first group's wait; then
// what the families compute once per stream-frame
DcsStatus EncRun::analyse()
{
    const uint32_t nStreams = in.nStreams;
    const uint64_t first = in.sampleOffsets[0], nSamples = in.sampleOffsets[nStreams] - first;
    bad.resize(nStreams);
    ENCCHK(hipMemcpyAsync(cb.dT, tabs, sizeof(EncTabs), hipMemcpyHostToDevice, st));
    if (!dev && !devF)
        ENCCHK(hipMemcpyAsync(cb.dPcm, in.hostPcm + first, sizeof(float) * nSamples, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(cb.dStr, hs.data(), sizeof(EncStream) * nStreams, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(cb.dSets, hsets.data(), sizeof(EncSet) * jobs.nSets, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(cb.dFS, frameStream.data(), sizeof(uint32_t) * F, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(cb.dBad, 0, sizeof(uint32_t) * nStreams, st));
    if (dev)
        hipLaunchKernelGGL(encAnalyseKernel<int16_t>, dim3((F + 3) / 4), dim3(256), 0, st, cb.dT, in.devPcm + first, cb.dStr, cb.dFS, F,
                           cb.dSpec, cb.dPw, cb.dLo, cb.dHi, cb.dBad, in.devErr);
    else
        hipLaunchKernelGGL(encAnalyseKernel<float>, dim3((F + 3) / 4), dim3(256), 0, st, cb.dT, devF ? in.devFloat + first : cb.dPcm,
                           cb.dStr, cb.dFS, F, cb.dSpec, cb.dPw, cb.dLo, cb.dHi, cb.dBad, static_cast<const uint32_t *>(nullptr));
    for (EncFamily *f : fams)
        ENCTRY(f->streamSums());
    ENCCHK(hipMemcpyAsync(bad.data(), cb.dBad, sizeof(uint32_t) * nStreams, hipMemcpyDeviceToHost, st));
    if (in.devStreamErr != nullptr)
    {
        decodeErr.resize(nStreams);
        ENCCHK(hipMemcpyAsync(decodeErr.data(), in.devStreamErr, sizeof(uint32_t) * nStreams, hipMemcpyDeviceToHost, st));
    }
    for (EncFamily *f : fams)
        ENCTRY(f->analyse());
    return DCS_OK;
}

// group g through the families up to the sizes, and a wait: win, keep and size of its jobs are on the host after it
DcsStatus EncRun::runGroup(uint32_t g)
{
    const uint32_t j0 = groupFirst[g], n = groupFirst[g + 1] - j0;
    hj.resize(n);
    frameJob.clear();
    uint32_t JF = 0;
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const DcsSweepJob &job = jobs.list[j0 + k];
        const EncStream &s = hs[job.stream];
        hj[k] = EncJob{ job.stream, job.paramSet, JF, s.nFrames, s.firstFrame };
        frameJob.insert(frameJob.end(), s.nFrames, k);
        JF += s.nFrames;
    }
    ENCCHK(hipMemcpyAsync(gb.dJobs, hj.data(), sizeof(EncJob) * n, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemcpyAsync(gb.dFJ, frameJob.data(), sizeof(uint32_t) * JF, hipMemcpyHostToDevice, st));
    for (EncFamily *f : fams)
        ENCTRY(f->runGroup(j0, n, JF));
    if (jobs.fit != nullptr && !fit.allotted)
        fit.launchCurves(j0, n);
    ENCCHK(hipGetLastError());
    for (EncFamily *f : fams)
        ENCTRY(f->fetchGroup(j0, n));
    ENCCHK(hipStreamSynchronize(st));
    for (EncFamily *f : fams)
        f->sizeJobs(j0, n);
    resident = g;
    residentFrames = JF;
    return DCS_OK;
}

// what the first wait brings: was the input usable at all (planFlag), then did E1 refuse a sample (bad[])
DcsStatus EncRun::checkInput()
{
    if (in.planFlag != nullptr && *in.planFlag != 0)
    {
        in.unusable = true;
        return DCS_ERR_BAD_STREAM;
    }
    for (uint32_t i = 0 ; i < in.nStreams ; ++i)
        if (bad[i] || (!decodeErr.empty() && decodeErr[i]))
        {
            dcsCtxSetError(ctx, (name(i) + (dev || (!decodeErr.empty() && decodeErr[i]) ? ": the decoder reports an error in a frame (DCS_FRAME_STOP / DCS_FRAME_FATAL)"
                                                : in.bound != nullptr ? ": a sample is not finite or beyond its format's full scale"
                                                : ": a sample is not finite or |x| > 1")).c_str());
            return DCS_ERR_BAD_STREAM;
        }
    return DCS_OK;
}

// info, the sweep's result and the families' records of job j, from what its group's run left on the host
void EncRun::writeInfo(uint32_t j)
{
    const DcsEncodeInfo e{ kCandType[win[j]], kCandSub[win[j]], static_cast<int32_t>(hs[jobs.list[j].stream].nFrames),
                           static_cast<int32_t>(size[j]), keep[j] };
    if (to.info != nullptr)
        to.info[j] = e;
    if (to.info93a != nullptr)
        to.info93a[j] = DcsEncode93aInfo{};     // (what a job of the A family's stays at for any other)
    for (EncFamily *f : fams)
        f->writeInfo(j);
    if (sweep.results != nullptr)
    {
        memset(&sweep.results[j], 0, sizeof(DcsSweepResult));       // (its padding too: records compare as bytes)
        sweep.results[j].enc = e;
    }
}

// every size is known: outOffsets, info and results, then dst (null with DCS_OK: a sweep that asked for sizes only).  (A fit
// call knows the sizes, its allotments, before its groups have chosen: fit.report writes their info.)
DcsStatus EncRun::placeOutput()
{
    uint64_t *outOffsets = to.outOffsets;
    for (uint32_t j = 0 ; j < jobs.n ; ++j)
    {
        outOffsets[j + 1] = outOffsets[j] + size[j];
        if (jobs.fit == nullptr)
            writeInfo(j);
    }
    if (sweep.sizesOnly)
        return DCS_OK;
    const uint64_t total = outOffsets[jobs.n];
    dst = to.place != nullptr && *to.place ? (*to.place)(outOffsets, total) : (to.out != nullptr && to.outCap >= total ? to.out : nullptr);
    return dst != nullptr ? DCS_OK : DCS_ERR_CAPACITY;
}

// Where the jobs of group g lie in its blob, and the blob's size in words.  For the output: as in the output.  For a
// decode: where the device path's stream layout wants them (each stream on a 4-byte boundary, the blob's zeroed tail).
DcsStatus EncRun::layoutGroup(uint32_t g, size_t *nWords)
{
    const uint32_t j0 = groupFirst[g], n = groupFirst[g + 1] - j0;
    offs.resize(n);
    if (!sweep.measure)
    {
        for (uint32_t k = 0 ; k < n ; ++k)
            offs[k] = to.outOffsets[j0 + k] - to.outOffsets[j0];
        blobLen = static_cast<size_t>(to.outOffsets[j0 + n] - to.outOffsets[j0]);
        *nWords = (blobLen + 3) / 4 + 1;
        return DCS_OK;
    }
    ss.resize(n);
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        // (an OS93 set has no subtype: buildSets admits only the candidates whose kCandSub is 0)
        const int c = win[j0 + k];
        const uint16_t ver = jobs.sets[hj[k].set].formatVersion;
        uint32_t head = 0;
        for (const EncFamily *f : fams)
            head |= f->head(j0 + k);
        ss[k] = DcsSweepStream{ hj[k].nFrames, static_cast<uint32_t>(size[j0 + k]),
                                ver == 0x9301 ? DCS_OS93A : ver == 0x9302 ? DCS_OS93B : kCandSub[c] == 3 ? DCS_OS95 : DCS_OS94, kCandType[c],
                                kCandSub[c], keep[j0 + k], head };
    }
    size_t blobBytes;
    ENCTRY(dcsSweepLayout(ss.data(), n, offs.data(), &blobLen, &blobBytes));
    *nWords = blobBytes / 4;
    return DCS_OK;
}

// header, pack and swap of the resident group g into a blob of its own
DcsStatus EncRun::packGroup(uint32_t g)
{
    const uint32_t n = groupFirst[g + 1] - groupFirst[g], JF = residentFrames;
    size_t nWords;
    ENCTRY(layoutGroup(g, &nWords));
    blob.clear();
    staged = false;
    ENCCHK(blob.alloc(&dW, nWords));
    ENCCHK(hipMemsetAsync(dW, 0, sizeof(uint32_t) * nWords, st));
    ENCCHK(hipMemcpyAsync(gb.dOutOff, offs.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice, st));
    for (EncFamily *f : fams)
        ENCTRY(f->packGroup(n, JF));
    hipLaunchKernelGGL(encSwapKernel, dim3(static_cast<unsigned>((nWords + 255) / 256)), dim3(256), 0, st, dW, nWords);
    ENCCHK(hipGetLastError());
    return DCS_OK;
}

// the packed group g to its place in the output, and a wait
DcsStatus EncRun::deliverGroup(uint32_t g)
{
    ENCCHK(hipMemcpyAsync(dst + to.outOffsets[groupFirst[g]], dW, blobLen, hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    return DCS_OK;
}

// the packed group's blob to `stage`, queued once per group; the caller waits
DcsStatus EncRun::stageBlob()
{
    if (staged)
        return DCS_OK;
    stage.resize(blobLen);
    ENCCHK(hipMemcpyAsync(stage.data(), dW, blobLen, hipMemcpyDeviceToHost, st));
    staged = true;
    return DCS_OK;
}

// The jobs of the packed group (n of them) whose streams are decoded.  One kind is left out: an OS93a Type-0 stream with
// no band kept.  Its header is sixteen 0xFF bytes, the first of which carries the type bit, so every decoder reads it as
// OS93a Type 1 with 31 bands; its record stays measured = 0.  (A Type-1 stream's header says what it is: always decoded.)
void EncRun::selectDecodes(uint32_t n)
{
    sel.clear(); selS.clear(); selOff.clear();
    mostFrames = 0;
    selFrames = 0;
    for (uint32_t k = 0 ; k < n ; ++k)
        if (!(ss[k].os == DCS_OS93A && ss[k].formatType == 0 && ss[k].bandsToKeep == 0))
        {
            sel.push_back(k); selS.push_back(ss[k]); selOff.push_back(offs[k]);
            mostFrames = std::max(mostFrames, hj[k].nFrames);
            selFrames += hj[k].nFrames;
        }
}

// One attempt: the selected streams decoded, on the device path from the bytes where they lie or (onHost) as a host-planned
// batch from the staged blob, then M1 and a wait, after which meas[] is on the host, and so is the blob where the output
// wants it.  *unusable: the device planner gave the list up (its flag); the sums are then not to be used.
DcsStatus EncRun::decodeAndCompare(uint32_t n, bool onHost, bool *unusable)
{
    if (onHost && !staged)
    {
        ENCTRY(stageBlob());
        ENCCHK(hipStreamSynchronize(st));
    }
    SweepDecodeGuard dec;
    const int16_t *decPcm = nullptr;
    const uint32_t *decErr = nullptr, *firstFrame = nullptr;
    const volatile uint32_t *flag = nullptr;
    const uint32_t nSel = static_cast<uint32_t>(sel.size());
    ENCTRY(dcsSweepDecodeStart(ctx, selS.data(), nSel, selOff.data(), reinterpret_cast<const uint8_t *>(dW), blobLen,
                               onHost ? stage.data() : nullptr, &dec.d, &decPcm, &decErr, &flag, &firstFrame));
    for (uint32_t i = 0 ; i < nSel ; ++i)
        firstDec[sel[i]] = firstFrame[i];
    ENCCHK(hipMemcpyAsync(dFirstDec, firstDec.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(dMeas, 0, sizeof(EncMeasure) * n, st));
    hipLaunchKernelGGL(encMeasureKernel, dim3(n, (mostFrames + 1 + kMeasureFrames - 1) / kMeasureFrames), dim3(256), 0, st,
                       cb.dPcm, cb.dStr, gb.dJobs, dFirstDec, decPcm, decErr, dMeas);
    ENCCHK(hipGetLastError());
    ENCCHK(hipMemcpyAsync(meas.data(), dMeas, sizeof(EncMeasure) * n, hipMemcpyDeviceToHost, st));
    if (dst != nullptr)
        ENCTRY(stageBlob());
    ENCCHK(hipStreamSynchronize(st));
    *unusable = flag != nullptr && *flag != 0;
    return DCS_OK;
}

// meas[] to the results of group g's jobs, and their bytes from `stage` to the output
DcsStatus EncRun::reportGroup(uint32_t g)
{
    const uint32_t j0 = groupFirst[g], n = groupFirst[g + 1] - j0;
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const uint32_t j = j0 + k;
        if (meas[k].err != 0)
        {
            dcsCtxSetError(ctx, ("job " + std::to_string(j) + " (" + name(hj[k].stream) + ", set " + std::to_string(hj[k].set)
                                 + "): the decoder reports an error in a frame of the stream just encoded").c_str());
            return DCS_ERR_HIP;
        }
        DcsSweepResult &r = sweep.results[j];
        if (dst != nullptr)
            memcpy(dst + to.outOffsets[j], stage.data() + offs[k], size[j]);
        if (firstDec[k] == kNotDecoded)
            continue;
        r.measured = 1;
        r.peakErr = meas[k].peak;
        r.nCompared = hs[hj[k].stream].nSamples;
        r.sumSrcSq = static_cast<int64_t>(meas[k].srcSq);
        r.sumDecSq = static_cast<int64_t>(meas[k].decSq);
        r.sumCross = static_cast<int64_t>(meas[k].cross);
    }
    return DCS_OK;
}

// The packed group g decoded and compared with its sources.  The decode, as transcoding runs it (dcs_transcode.hip.h): the
// device path on the bytes where they lie; the host-planned batch, for which the bytes are read back, where the device
// planner cannot serve the list (a second attempt) or one long stream dominates it (the only one: the device index walk is
// one wavefront per stream, serial over its frames).
DcsStatus EncRun::measureGroup(uint32_t g)
{
    const uint32_t n = groupFirst[g + 1] - groupFirst[g];
    selectDecodes(n);
    const bool walkOnHost = mostFrames > 2048 && uint64_t(mostFrames) * 64 > selFrames;
    meas.assign(n, EncMeasure{});
    firstDec.assign(n, kNotDecoded);
    if (sel.empty() && dst != nullptr)
    {
        ENCTRY(stageBlob());
        ENCCHK(hipStreamSynchronize(st));
    }
    for (int attempt = walkOnHost ? 1 : 0 ; attempt < 2 && !sel.empty() ; ++attempt)
    {
        bool unusable = false;
        ENCTRY(decodeAndCompare(n, attempt == 1, &unusable));
        if (!unusable)
            break;
    }
    return reportGroup(g);
}

DcsStatus EncRun::run()
{
    ENCTRY(checkStreams());
    to.outOffsets[0] = 0;
    if (in.nStreams == 0 || jobs.n == 0)
    {
        for (uint32_t j = 0 ; j < jobs.n ; ++j)
            to.outOffsets[j + 1] = 0;
        return DCS_OK;
    }
    buildSets();
    win.resize(jobs.n); keep.resize(jobs.n); size.resize(jobs.n);
    ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
    ENCTRY(allocCall());
    ENCTRY(allocGroups());
    ENCTRY(analyse());
    const uint32_t nGroups = static_cast<uint32_t>(groupFirst.size()) - 1;
    for (uint32_t g = 0 ; g < nGroups ; ++g)
    {
        ENCTRY(runGroup(g));
        if (g == 0)
            ENCTRY(checkInput());
    }
    if (jobs.fit != nullptr)
        ENCTRY(fit.allot());
    ENCTRY(placeOutput());
    if (dst == nullptr && !sweep.measure)
        return DCS_OK;
    for (uint32_t g = 0 ; g < nGroups ; ++g)
    {
        if (jobs.fit != nullptr)
        {
            ENCTRY(nGroups == 1 ? fit.rechoose(g) : runGroup(g));
            for (uint32_t j = groupFirst[g] ; j < groupFirst[g + 1] ; ++j)
            {
                ENCTRY(fit.report(j));
                writeInfo(j);
            }
        }
        else if (resident != g)
            ENCTRY(runGroup(g));
        ENCTRY(packGroup(g));
        ENCTRY(sweep.measure ? measureGroup(g) : deliverGroup(g));
    }
    if (jobs.fit != nullptr)
        fit.record();
    return DCS_OK;
}

// ------------------------------------------------------------------------------------------- what the entry points share

// every stream with one parameter set, job i = (stream i, set 0); with the caller's PCM on the host as the input, where the
// caller has no input of its own
struct EncOneSet
{
    explicit EncOneSet(uint32_t nStreams) : list(nStreams)
    {
        for (uint32_t i = 0 ; i < nStreams ; ++i)
            list[i] = DcsSweepJob{ i, 0 };
    }
    EncOneSet(const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams) : EncOneSet(nStreams)
    {
        in.sampleOffsets = sampleOffsets;
        in.nStreams = nStreams;
        in.hostPcm = pcm;
    }
    EncJobs jobs(const DcsEncodeParams *params, bool os93) const
    {
        return EncJobs{ params, 1, list.data(), static_cast<uint32_t>(list.size()), os93 };
    }
    EncInput in;
    std::vector<DcsSweepJob> list;
};

// the entry points that encode every stream of an input with one parameter set
DcsStatus encodeStreams(DcsCtx *ctx, EncInput &in, const DcsEncodeParams *params, bool os93, const EncOutput &to)
{
    const bool dev = in.devPcm != nullptr, devF = in.devFloat != nullptr;
    if (ctx == nullptr || in.sampleOffsets == nullptr || to.outOffsets == nullptr
        || (in.nStreams != 0 && in.hostPcm == nullptr && !dev && !devF) || (dev && in.devErr == nullptr))
        return DCS_ERR_INVALID_ARG;
    if (!paramsValid(params, os93))
    {
        if (const char *why = whyOs93aType1(params, os93))
            dcsCtxSetError(ctx, why);
        return DCS_ERR_INVALID_ARG;
    }
    return EncRun(ctx, in, EncOneSet(in.nStreams).jobs(params, os93), to, EncSweep()).run();
}

// dcs_encode_streams and dcs_encode93_streams
DcsStatus encodeHostPcm(DcsCtx *ctx, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams, const DcsEncodeParams *params,
                        bool os93, const EncOutput &to)
{
    EncInput in;
    in.sampleOffsets = sampleOffsets;
    in.nStreams = nStreams;
    in.hostPcm = pcm;
    return encodeStreams(ctx, in, params, os93, to);
}

// a set of the searched family that `os93` names (R or S); `say` takes the message of one that is not, `fn` the call's name
bool searchedParams(const char *fn, const DcsEncodeParams *params, bool os93, const std::function<void(const char *)> &say)
{
    if (os93 ? paramsValid93Rd(params) : paramsValidRd(params))
        return true;
    say((std::string(fn) + (os93 ? ": formatVersion 0x9301 or 0x9302, streamFormatType 0 or -1 (OS93 Type 0; Type 1 is "
                                   "not searched), targetBitRate 1..100 000 000 and finite parameters"
                                 : ": formatVersion 0x9400, streamFormatType 0, 1 or -1, streamFormatSubType 0, 3 or -1, "
                                   "targetBitRate 1..100 000 000 and finite parameters")).c_str());
    return false;
}

// The search on any input, the one place that makes a searched EncJobs: job j = (stream list[j].stream, the one set), searched
// to budgetBytes[j] (null: the set's targetBitRate) or, all jobs together, to `fit`.  The set has passed searchedParams.
DcsStatus searchInput(DcsCtx *ctx, EncInput &in, const std::vector<DcsSweepJob> &list, const DcsEncodeParams *params, bool os93,
                      const uint32_t *budgetBytes, const EncFit *fit, const EncOutput &to)
{
    if (fit != nullptr && fit->info != nullptr)
    {
        *fit->info = DcsEncodeRdFitInfo{};
        fit->info->totalBytes = fit->totalBytes;
        fit->info->fits = 1;
    }
    EncJobs js{ params, 1, list.data(), static_cast<uint32_t>(list.size()), os93 };
    js.search = true;
    js.budgetBytes = budgetBytes;
    js.fit = fit;
    return EncRun(ctx, in, js, to, EncSweep()).run();
}

// dcs_encode_rd_streams, dcs_encode93_rd_streams, dcs_encode_rd_fit and dcs_encode93_rd_fit (`fn`: which, for the message):
// the null arguments they refuse, then a set that is not one of the family that `os93` names; then the call, every stream
// of the caller's host PCM searched with the one set, to budgetBytes or to `fit`
DcsStatus encodeSearched(DcsCtx *ctx, const char *fn, const float *pcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                         const DcsEncodeParams *params, bool os93, const uint32_t *budgetBytes, const EncFit *fit, uint8_t *out,
                         uint64_t outCap, uint64_t *outOffsets, DcsEncodeInfo *info, DcsEncodeRdInfo *infoRd)
{
    if (ctx == nullptr || sampleOffsets == nullptr || outOffsets == nullptr || (nStreams != 0 && pcm == nullptr))
        return DCS_ERR_INVALID_ARG;
    if (!searchedParams(fn, params, os93, [&](const char *why) { dcsCtxSetError(ctx, why); }))
        return DCS_ERR_INVALID_ARG;
    EncOneSet one(pcm, sampleOffsets, nStreams);
    EncOutput to{ out, static_cast<size_t>(outCap), outOffsets, info, nullptr, nullptr };
    to.infoRd = infoRd;
    return searchInput(ctx, one.in, one.list, params, os93, budgetBytes, fit, to);
}

// ---------------------------------------------------------------------- budgets from any source

// os93 as the calls that take any target read it
bool budgetOs93(const DcsEncodeParams *params) { return params != nullptr && params->formatVersion != 0x9400; }

// the DcsBudget of a call: there, and budgetBytes only in the per-job form
bool budgetValid(const char *fn, const DcsBudget *b, const std::function<void(const char *)> &say)
{
    if (b == nullptr)
        return false;
    if (b->shared > 1 || (b->shared != 0 && b->budgetBytes != nullptr))
    {
        say((std::string(fn) + (b->shared > 1 ? ": budget->shared is 0 (one budget per job) or 1 (one budget for the set)"
                                              : ": budget->budgetBytes is for the per-job form; the shared form takes totalBytes and capBytes")).c_str());
        return false;
    }
    return true;
}

// is a source that fits the target's family copied under `b`?  Unit i of the call.
bool budgetCopies(const DcsBudget &b, uint32_t i, uint64_t len)
{
    const uint32_t *most = b.shared != 0 ? b.capBytes : b.budgetBytes;
    return most == nullptr || len <= most[i];
}

// The units of a budget call (streams or files, in input order): each is a job that is searched, or a copy of bytes that
// exist.  copy[i] null: searched, and stream[i] is its stream of the EncInput.
struct BudgetUnits
{
    std::vector<const uint8_t *> copy;
    std::vector<uint64_t> copyLen;
    std::vector<uint32_t> stream;
    uint32_t n() const { return static_cast<uint32_t>(copy.size()); }
    void search(uint32_t s) { copy.push_back(nullptr); copyLen.push_back(0); stream.push_back(s); }
    void keep(const uint8_t *p, uint64_t len) { copy.push_back(p); copyLen.push_back(len); stream.push_back(0); }
};

// What the three budget calls share behind their sources: the searched units of `u` as the jobs of ONE EncRun on `in`, with
// their share of `b` (per job: their own budgets; shared: the total less the copies, their own caps), then the units' layout
// in input order, the capacity, the copies' bytes and the records.  enc[i]: unit i's DcsEncodeInfo where it was searched
// (the caller's own record type takes it).  On DCS_ERR_CAPACITY outOffsets, infoRd (per-job form) and *b.fit stand.
DcsStatus encodeBudgeted(DcsCtx *ctx, EncInput &in, const BudgetUnits &u, const DcsEncodeParams *params, bool os93, const DcsBudget &b,
                         uint8_t *out, size_t outCap, uint64_t *outOffsets, std::vector<DcsEncodeInfo> &enc, DcsEncodeRdInfo *infoRd)
{
    const uint32_t n = u.n();
    std::vector<DcsSweepJob> list;
    std::vector<uint32_t> unitOf, budgets, caps;
    uint64_t copied = 0;
    for (uint32_t i = 0 ; i < n ; ++i)
        if (u.copy[i] == nullptr)
        {
            list.push_back(DcsSweepJob{ u.stream[i], 0 });
            unitOf.push_back(i);
            if (b.budgetBytes != nullptr)
                budgets.push_back(b.budgetBytes[i]);
            if (b.capBytes != nullptr)
                caps.push_back(b.capBytes[i]);
        }
        else
            copied += u.copyLen[i];
    const uint32_t nS = static_cast<uint32_t>(list.size());
    // (a shared total that the copies alone exceed leaves the searched jobs nothing: 10.13's rule 4 on what is left)
    DcsEncodeRdFitInfo rec{};
    const EncFit fit{ b.totalBytes > copied ? b.totalBytes - copied : 0, b.capBytes != nullptr ? caps.data() : nullptr, &rec };
    std::vector<DcsEncodeInfo> encS(nS);
    std::vector<DcsEncodeRdInfo> rdS(nS);
    std::vector<uint64_t> offS(static_cast<size_t>(nS) + 1, 0);
    std::vector<uint8_t> bytes;
    const auto layout = [&](const uint64_t *offs) -> uint64_t {
        outOffsets[0] = 0;
        for (uint32_t i = 0, k = 0 ; i < n ; ++i)
        {
            outOffsets[i + 1] = outOffsets[i] + (u.copy[i] != nullptr ? u.copyLen[i] : offs[k + 1] - offs[k]);
            k += u.copy[i] == nullptr ? 1 : 0;
        }
        return outOffsets[n];
    };
    const EncPlace place = [&](const uint64_t *offs, uint64_t total) -> uint8_t * {
        if (layout(offs) > outCap || out == nullptr)
            return nullptr;
        if (nS == n)                            // no copy: the searched streams' layout is the call's, straight into `out`
            return out;
        bytes.resize(total ? total : 1);
        return bytes.data();
    };
    DcsStatus st = DCS_OK;
    if (nS != 0)
    {
        EncOutput to{ nullptr, 0, offS.data(), encS.data(), &place, nullptr };
        to.infoRd = rdS.data();
        st = searchInput(ctx, in, list, params, os93, b.shared == 0 && b.budgetBytes != nullptr ? budgets.data() : nullptr,
                         b.shared != 0 ? &fit : nullptr, to);
    }
    else
    {
        rec.fits = 1;
        if (layout(offS.data()) > outCap || (n != 0 && out == nullptr))
            st = DCS_ERR_CAPACITY;
    }
    if (st != DCS_OK && st != DCS_ERR_CAPACITY)
        return st;
    if (b.shared != 0 && b.fit != nullptr)
    {
        rec.totalBytes = b.totalBytes;
        rec.leastBytes += copied;
        rec.usedBytes += copied;
        rec.fits = rec.leastBytes <= b.totalBytes ? 1 : 0;
        *b.fit = rec;
    }
    // (the searched records as far as the driver wrote them: all of them in the per-job form, none before a shared call's
    // capacity was looked at)
    enc.assign(n, DcsEncodeInfo{});
    for (uint32_t i = 0, k = 0 ; i < n ; ++i)
    {
        DcsEncodeRdInfo r{};
        r.fits = 1;
        if (u.copy[i] == nullptr)
        {
            enc[i] = encS[k];
            r = rdS[k++];
        }
        if (infoRd != nullptr)
            infoRd[i] = r;
    }
    if (st != DCS_OK)
        return st;
    for (uint32_t i = 0, k = 0 ; nS != n && i < n ; ++i)
        if (u.copy[i] != nullptr)
            memcpy(out + outOffsets[i], u.copy[i], u.copyLen[i]);
        else
        {
            memcpy(out + outOffsets[i], bytes.data() + offS[k], offS[k + 1] - offS[k]);
            ++k;
        }
    return DCS_OK;
}

}  // namespace
