// dcs_plan_device.hip.h -- the chunk planner and the chunk packer on the device, and the host code that queues them.
// Part of the translation unit dcs_runtime.hip (included there once the batch and its buffers are declared).  What a plan and a
// package hold is stated in dcs_package.h; the kernels here decide only how the work is spread over threads and lanes.

// ---------------------------------------------------------------------------------------------------------
// The packer on the device: the same packages dcsBuildPackages (dcs_plan.cpp) lays out on the host, assembled by one
// wavefront per chunk from what is already resident -- the index records the device index pass left there, the streams
// as uploaded for that pass -- and the plan the host made from an 8-byte-per-frame digest.  Byte for byte the same
// packages (tests/test_gpu_corpus.py compares them).
// ---------------------------------------------------------------------------------------------------------
namespace {
template <int FPW>
__global__ __launch_bounds__(256) void dcsPackKernel(const DcsSlot *slots, uint32_t nChunks, const DcsPlanSrc *srcs,
                                                      const DcsFrameIndex *records, const uint8_t *blob, uint64_t blobLen,
                                                      uint8_t *packages, uint32_t layout)
{
    const uint32_t chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = static_cast<int>(threadIdx.x & 63);
    if (chunk >= nChunks)
        return;
    uint8_t *pkg = packages + static_cast<size_t>(chunk) * dcsPkgStride(FPW, layout);
    const DcsSlot *cs = slots + static_cast<size_t>(chunk) * FPW;
    const uint32_t imgDw = dcsPkgImgDw(layout);
    // (order: the image first -- its loads need nothing but the plan's slots, and a wavefront issues its loads in program order: behind the
    // slot -> source -> record chain of the descriptors they waited for three round trips before they were even asked for)
    // the image of the bit pool: the chunk's runs of stream dwords; zero between them (the runs lie one behind the other, each on
    // a 16-byte boundary: gaps of at most three dwords) and behind the last one
    uint32_t *img = reinterpret_cast<uint32_t *>(pkg + dcsPkgOffPool(FPW, layout));
    uint32_t end = 0;
    for (int k = 0 ; k < FPW ; ++k)
    {
        const uint32_t n = cs[k].runNDw, st = cs[k].runStartDw, o = cs[k].runPoolOff;
        if (n == 0)
            break;
        if (o + n > imgDw || o < end)
            continue;                           // (cannot happen: the image covers every run of the plan, in order)
        for (uint32_t i = end + static_cast<uint32_t>(lane) ; i < o ; i += 64)
            img[i] = 0;
        // (four dwords a lane where the run and the blob have them: the run starts on a 16-byte boundary of the image, the stream
        // bytes on a dword boundary only)
        const uint32_t n4 = (static_cast<uint64_t>(st) + n) * 4 <= blobLen ? n & ~3u : 0u;
        for (uint32_t i = static_cast<uint32_t>(lane) * 4 ; i < n4 ; i += 256)
        {
            const uint64_t dw = static_cast<uint64_t>(st) + i;
            const uint32_t w0 = dcsImageDwordInside(blob, dw), w1 = dcsImageDwordInside(blob, dw + 1);
            const uint32_t w2 = dcsImageDwordInside(blob, dw + 2), w3 = dcsImageDwordInside(blob, dw + 3);
            *reinterpret_cast<uint4 *>(img + o + i) = make_uint4(w0, w1, w2, w3);
        }
        for (uint32_t i = n4 + static_cast<uint32_t>(lane) ; i < n ; i += 64)
            img[o + i] = dcsImageDword(blob, blobLen, static_cast<uint64_t>(st) + i);
        end = o + n;
    }
    {
        // (behind the last run: dwords up to the next 16-byte boundary, then sixteen bytes a lane)
        const uint32_t end4 = (end + 3u) & ~3u;
        for (uint32_t i = end + static_cast<uint32_t>(lane) ; i < end4 && i < imgDw ; i += 64)
            img[i] = 0;
        for (uint32_t i = end4 + static_cast<uint32_t>(lane) * 4 ; i + 4 <= imgDw ; i += 256)
            *reinterpret_cast<uint4 *>(img + i) = make_uint4(0, 0, 0, 0);
        for (uint32_t i = (imgDw & ~3u) + static_cast<uint32_t>(lane) ; i < imgDw ; i += 64)
            if (i >= end4)
                img[i] = 0;
    }
    // EVERY byte of the package is written here, once (round 5: the buffer used to be cleared first, 700 MB of writes in front of
    // the packer for 2 M frames): what does not apply is written as zero, as the host packer's memset leaves it.
    // slot `lane`: its entry of five 16-byte pieces
    if (lane < FPW)
    {
        const DcsSlot sl = cs[lane];
        uint32_t e[DCS_PKG_SLOT_DWORDS];
        dcsPkgSlotEntry(e, sl, dcsPkgSrcOf(sl, srcs, records), blob, blobLen);
        uint4 *ps = reinterpret_cast<uint4 *>(pkg + static_cast<size_t>(lane) * DCS_PKG_SLOT_BYTES);
#pragma unroll
        for (int i = 0 ; i < DCS_PKG_SLOT_DWORDS / 4 ; ++i)
            ps[i] = make_uint4(e[4 * i], e[4 * i + 1], e[4 * i + 2], e[4 * i + 3]);
    }
    // the lane's own record: the split record of the frame's q-th unpack lane (zero where there is none)
    {
        const DcsSlot sl = cs[lane % FPW];
        uint32_t r[2];
        dcsLaneSplit(r, dcsPkgSrcOf(sl, srcs, records), sl.bpl, lane / FPW, 64 / FPW);
        if (layout & DCS_PKG_SPLIT4)
            reinterpret_cast<uint32_t *>(pkg + dcsPkgOffSplit(FPW))[lane] = dcsLaneSplit4(r);
        else
            reinterpret_cast<uint2 *>(pkg + dcsPkgOffSplit(FPW))[lane] = make_uint2(r[0], r[1]);
    }
    // (the bytes between the split records and the image's 128-byte boundary)
    {
        const uint32_t padFrom = dcsPkgOffSplit(FPW) + 64u * dcsPkgSplitBytes(layout), padTo = dcsPkgOffPool(FPW, layout);
        for (uint32_t i = padFrom / 4 + static_cast<uint32_t>(lane) ; i < padTo / 4 ; i += 64)
            reinterpret_cast<uint32_t *>(pkg)[i] = 0;
    }
}
}   // namespace

// ---------------------------------------------------------------------------------------------------------
// The planner on the device, for lists of WHOLE STREAMS (the pipeline's third step onto the device: the index records never
// leave it, and the host neither waits for them nor plans).  One thread per chunk works the arithmetic plan of its chunk out
// (dcsPlanChunk, dcs_package.h) and writes the chunk's slots; what that plan cannot express is raised in a flag word, and the
// list then takes the host planner's path.
// ---------------------------------------------------------------------------------------------------------
namespace {
template <int FPW>
__global__ __launch_bounds__(256) void dcsPlanKernel(const DcsPlanStream *streams, uint32_t nStreams, uint32_t extraFrames, uint32_t nJobs,
                                                      const DcsFrameIndex *records, const DcsStreamInfo *infos,
                                                      DcsSlot *slots, DcsPlanSrc *srcs, uint32_t *flagWord, uint32_t *hostFlag, uint32_t fpc)
{
    const uint32_t nChunks = (nJobs + fpc - 1) / fpc;
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nChunks)
        return;
    DcsSlot out[FPW];
    const uint32_t flags = dcsPlanChunk<FPW>(streams, nStreams, infos, records, extraFrames, nJobs, fpc, c, out, srcs);
    for (int p = 0 ; p < FPW ; ++p)
        slots[static_cast<size_t>(c) * FPW + p] = out[p];
    if (flags != 0)
    {
        const uint32_t seen = atomicOr(flagWord, flags);
        // ... and straight into the batch's pinned staging word, so that no copy kernel has to bring it down behind the decode
        // launch.  A plain store of everything this thread knows raised (its own bits and those the device word held before):
        // non-zero is all the host needs for the PCM to be safe; concurrent writers can still hide each other's bits, which
        // is why the host retries only on "overflow and NOT truncated" and treats the word as "at least these" 
        if (hostFlag != nullptr)
            __hip_atomic_store(hostFlag, seen | flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
}   // namespace

// one wavefront per chunk, four to a workgroup (dcsPackKernel above)
static hipError_t launchPack(int fpw, hipStream_t stream, const DcsSlot *slots, uint32_t nChunks, const DcsPlanSrc *srcs, const DcsFrameIndex *records,
                             const uint8_t *blob, uint64_t blobLen, uint8_t *packages, uint32_t layout)
{
    withFpw(fpw, [&](auto w) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL(dcsPackKernel<W>, dim3((nChunks + 3) / 4), dim3(256), 0, stream, slots, nChunks, srcs, records, blob, blobLen, packages, layout);
    });
    return hipGetLastError();
}

namespace {
// three ranges cleared by one launch: a (16-byte units), b (dwords), c (16-byte units)
__global__ __launch_bounds__(256) void dcsClear3Kernel(uint4 *a, size_t nA16, uint32_t *b, size_t nB4, uint4 *c, size_t nC16)
{
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x, t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (size_t i = t ; i < nA16 ; i += stride) a[i] = z;
    for (size_t i = t ; i < nB4 ; i += stride) b[i] = 0;
    for (size_t i = t ; i < nC16 ; i += stride) c[i] = z;
}
}   // namespace

// What a planned-on-device batch (createBatchPlannedOnDevice, dcs_runtime.hip) queues in front of its decode launch: error words and hand-off words cleared,
// one thread per chunk plans (dcsPlanKernel), one wavefront per chunk packs (dcsPackKernel).  `between` (optional) is
// recorded between planner and packer (the device-path timing, dcs_device_path_run).
static DcsStatus queuePlanAndPack(DcsBatch *b, uint32_t nStreams, uint32_t extraFrames, const DcsFrameIndex *dRecords, const DcsStreamInfo *dInfos,
                                  const uint8_t *dBlob, uint64_t blobLen, hipEvent_t between)
{
    DcsCtx *ctx = b->ctx;
    const uint32_t nJobs = b->nJobs;
    // error words and hand-off words cleared by ONE kernel (three hipMemsetAsync were three dispatches in a chain of
    // ten per list; epoch 0 = never written; the planner's flag word lies behind the last chunk's hand-off words)
    {
        // (the packages are no longer among them: the pack kernel writes every byte of a package itself)
        const size_t errBytes = sizeof(uint32_t) * nJobs, hoBytes = b->dHandoff.bytes();
        const size_t total16 = (errBytes + 15) / 16 + hoBytes / 16;
        const unsigned blocks = static_cast<unsigned>(std::min<size_t>((total16 + 255) / 256, 2048));
        hipLaunchKernelGGL(dcsClear3Kernel, dim3(blocks), dim3(256), 0, b->stream, static_cast<uint4 *>(nullptr), static_cast<size_t>(0),
                           b->dErr, errBytes / 4, b->dHandoff.as<uint4>(), hoBytes / 16);
        HIPCHK(ctx, hipGetLastError());
    }
    uint32_t *flagWord = reinterpret_cast<uint32_t *>(b->dHandoff.as<unsigned long long>() + static_cast<size_t>(b->nChunks) * 16) + 2;
    const uint32_t planBlocks = (b->nChunks + 63) / 64;         // (one wavefront per workgroup: a thread's work is serial, the chunks should spread over the CUs)
    DcsSlot *dS = b->dPlanSlots.as<DcsSlot>();
    DcsPlanSrc *dP = b->dPlanSrcs.as<DcsPlanSrc>();
    withFpw(b->fpw, [&](auto w) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL(dcsPlanKernel<W>, dim3(planBlocks), dim3(64), 0, b->stream, b->dTable.as<const DcsPlanStream>(), nStreams, extraFrames, nJobs,
                           dRecords, dInfos, dS, dP, flagWord, b->hStage.as<uint32_t>(), b->planFpc);
    });
    HIPCHK(ctx, hipGetLastError());
    if (between != nullptr)
        HIPCHK(ctx, hipEventRecord(between, b->stream));
    HIPCHK(ctx, launchPack(b->fpw, b->stream, dS, b->nChunks, dP, dRecords, dBlob, blobLen, b->dPackages.as<uint8_t>(), b->imgDw));
    return DCS_OK;
}

// The device planner's stream table (DcsPlanStream, 40 bytes a stream): what the host knows of every stream of a list of
// whole streams without walking it -- where it lies in the list's blob, its layout, frame count, and the mixing parameters
// of frame 0 and of every later frame -- and the list's totals.
struct DcsPlanTable
{
    std::vector<DcsPlanStream> streams;
    uint64_t nJobs = 0;                 // output frames
    uint64_t payload = 0;               // bytes of the streams, headers included
    bool all94 = true, has93aT1 = false;
};
// ... made from the streams as laid out in the list's blob (layoutStreams); also the first output frame of every stream (n + 1 entries)
static DcsStatus planTableFor(const DcsStreamRef *streams, uint32_t n, uint32_t extraFrames, const DcsStreamLoc *locs, const uint64_t *firstRecord,
                              uint64_t totalRec, DcsPlanTable &table, std::vector<uint32_t> &firstJob)
{
    table.streams.resize(n);
    firstJob.resize(static_cast<size_t>(n) + 1);
    uint64_t nJobs = 0, payload = 0;
    bool all94 = true, has93a = false;
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const DcsStreamRef &sr = streams[k];
        const uint8_t *d = sr.data;
        const uint32_t len = locs[k].len;
        const uint32_t nFrames = (static_cast<uint32_t>(d[0]) << 8) | d[1];
        const bool typeBit = (d[2] & 0x80) != 0;
        const uint32_t h12 = (len > 3 ? d[3] : 0u) | (len > 4 ? d[4] : 0u);
        const DcsOsVersion os = static_cast<DcsOsVersion>(sr.os);
        DcsPlanStream &t = table.streams[k];
        t = DcsPlanStream{};
        t.hdrLen = (os == DCS_OS93A && typeBit) ? 1 : 16;
        t.format = static_cast<uint8_t>(os == DCS_OS93A ? (typeBit ? DCS_FMT_93A_T1 : DCS_FMT_93_T0)
                                      : os == DCS_OS93B ? (typeBit ? DCS_FMT_93B_T1 : DCS_FMT_93_T0)
                                      : !typeBit ? DCS_FMT_94_T0 : (h12 & 0x80) == 0 ? DCS_FMT_94_T1_S0 : DCS_FMT_94_T1_S3);
        t.xform = (os == DCS_OS93A || os == DCS_OS93B) ? DCS_XFORM_93 : DCS_XFORM_94;
        all94 = all94 && t.xform == DCS_XFORM_94;
        has93a = has93a || t.format == DCS_FMT_93A_T1;
        t.streamOff = locs[k].off;
        t.len = len;
        t.firstRecord = static_cast<uint32_t>(firstRecord[k]);
        t.firstJob = static_cast<uint32_t>(nJobs);
        t.nFrames = nFrames;
        uint16_t mm[2]; uint8_t vs[2];
        const DcsStatus st = dcs_stream_params_from(os, sr.volume, sr.level, sr.channelVolume, 0x7FFF, 2, mm, vs);    // frame 0, and every later frame
        if (st != DCS_OK)
            return st;
        t.mixMul0 = mm[0]; t.mixMulN = mm[1]; t.volShift0 = vs[0]; t.volShiftN = vs[1];
        firstJob[k] = static_cast<uint32_t>(nJobs);
        nJobs += nFrames + extraFrames;
        payload += len;
    }
    firstJob[n] = static_cast<uint32_t>(nJobs);
    table.nJobs = nJobs; table.payload = payload; table.all94 = all94; table.has93aT1 = has93a;
    return nJobs > 0xFFFFFFFFull || totalRec > 0xFFFFFFFFull ? DCS_ERR_CAPACITY : DCS_OK;
}

// Diagnostic / test entry: the packages of `jobs` as the DEVICE packer lays them out (plan from source digests on the
// host, pack kernel on the device), for comparison with dcs_pack_chunks, the host packer.  out = NULL to size.
extern "C" DcsStatus dcs_pack_chunks_device(DcsCtx *ctx, const DcsFrameJob *jobs, uint32_t nJobs, const DcsSrcDesc *srcs, uint32_t nSrcs,
                                            const uint8_t *blob, size_t blobLen, int fpw,
                                            uint8_t *out, size_t cap, uint32_t *nChunksOut, uint32_t *packageBytesOut)
{
    if (ctx == nullptr || jobs == nullptr || srcs == nullptr || blob == nullptr || nChunksOut == nullptr || !(fpw == 4 || fpw == 8 || fpw == 16))
        return DCS_ERR_INVALID_ARG;
    std::vector<DcsPlanSrc> ps(nSrcs);
    std::vector<DcsFrameIndex> recs(nSrcs);
    for (uint32_t k = 0 ; k < nSrcs ; ++k)
    {
        const DcsSrcDesc &sd = srcs[k];
        ps[k] = DcsPlanSrc{ sd.streamOff, sd.idx.bitOff, sd.idx.nBits, sd.hdrLen, sd.idx.nBands, sd.idx.flags, sd.format, sd.mixMul, k };
        recs[k] = sd.idx;
    }
    std::vector<DcsSlot> slots;
    const DcsPlan plan = dcsPlanJobs(jobs, nJobs, ps.data(), fpw, slots, DcsPlanOptions{ true, 0, false, DCS_MI355X_WAVE_PLACES });
    const uint32_t nChunks = *nChunksOut = plan.nChunks;
    uint32_t imgDw = plan.imgDw;
    if (dcsAllSources94(jobs, nJobs, srcs))
        imgDw |= DCS_PKG_SPLIT4;
    if (packageBytesOut != nullptr)
        *packageBytesOut = dcsPkgStride(fpw, imgDw);
    if (out == nullptr)
        return DCS_OK;
    const size_t pkgBytes = static_cast<size_t>(nChunks) * dcsPkgStride(fpw, imgDw);
    if (cap < pkgBytes)
        return DCS_ERR_CAPACITY;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    GrowBuf dSlots, dPs, dRecs, dBlob, dPkg;    // (outside the cache: a diagnostic entry's temporaries, freed when they go)
    const size_t blobAlloc = deviceBlobBytes(blobLen);
    const DcsStatus st = [&]() -> DcsStatus {
        HIPCHK(ctx, dSlots.room(sizeof(DcsSlot) * slots.size()));
        HIPCHK(ctx, dPs.room(sizeof(DcsPlanSrc) * (nSrcs ? nSrcs : 1)));
        HIPCHK(ctx, dRecs.room(sizeof(DcsFrameIndex) * (nSrcs ? nSrcs : 1)));
        HIPCHK(ctx, dBlob.room(blobAlloc));
        HIPCHK(ctx, dPkg.room(pkgBytes));
        HIPCHK(ctx, hipMemsetAsync(dBlob.as(), 0, blobAlloc, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(dPkg.as(), 0xA5, pkgBytes, ctx->stream));    // (the pack kernel writes every byte: a pattern it must leave nothing of)
        HIPCHK(ctx, hipMemcpyAsync(dSlots.as(), slots.data(), sizeof(DcsSlot) * slots.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(dPs.as(), ps.data(), sizeof(DcsPlanSrc) * nSrcs, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(dRecs.as(), recs.data(), sizeof(DcsFrameIndex) * nSrcs, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(dBlob.as(), blob, blobLen, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, launchPack(fpw, ctx->stream, dSlots.as<const DcsSlot>(), nChunks, dPs.as<const DcsPlanSrc>(), dRecs.as<const DcsFrameIndex>(),
                               dBlob.as<const uint8_t>(), blobLen, dPkg.as<uint8_t>(), imgDw));
        HIPCHK(ctx, hipMemcpyAsync(out, dPkg.as(), pkgBytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return DCS_OK;
    }();
    (void)hipStreamSynchronize(ctx->stream);    // (on failure too: queued copies may still be using the buffers that now go)
    return st;
}
