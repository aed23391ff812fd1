// dcs_large_list.hip.h -- dcs_decode_streams for a LARGE list: one synchronous call whose list goes, cut into parts, through a
// pipeline the context keeps for the purpose.  Included at the end of dcs_pipeline.hip.h, whose pipelineCreate, pipelineSubmit and
// dcs_pipeline_collect it drives as any caller would; of the pipeline's inside it sets roundGather and reads the two finish times.
#pragma once

static constexpr uint32_t kParts = 8;

// Cutting the list: part r is the streams cut[r] .. cut[r + 1], its share of the frames weight[r] of the weights' sum; first[k] is the
// first frame of stream k (nStreams + 1 entries).  Every part keeps at least one stream (nStreams >= 4 * kParts).
static void cutIntoParts(const std::vector<uint64_t> &first, const uint32_t *weight, uint32_t *cut)
{
    const uint32_t nStreams = static_cast<uint32_t>(first.size() - 1);
    uint32_t wSum = 0, wAcc = 0;
    for (uint32_t r = 0 ; r < kParts ; ++r)
        wSum += weight[r];
    cut[0] = 0;
    for (uint32_t r = 1 ; r < kParts ; ++r)
    {
        wAcc += weight[r - 1];
        const uint64_t target = first[nStreams] * wAcc / wSum;
        uint32_t k = static_cast<uint32_t>(std::lower_bound(first.begin(), first.end(), target) - first.begin());
        k = std::max(k, cut[r - 1] + 1);
        k = std::min(k, nStreams - (kParts - r));
        cut[r] = k;
    }
    cut[kParts] = nStreams;
}

// The walk shared with the device, after a call in which the host pool walked `hostParts` parts: who finished later?  (the pool's
// parts are submitted as they are walked, so both times are of lists of this call)  That side gets less in the next call.
static void adjustSharedHostParts(DcsCtx *ctx, DcsStatus st, double tCall0, uint32_t hostParts)
{
    double tHost, tDev;
    {
        std::lock_guard<std::mutex> lk(ctx->internalPipe->m);
        tHost = ctx->internalPipe->lastHostWalkedDone - tCall0;
        tDev = ctx->internalPipe->lastDeviceWalkedDone - tCall0;
    }
    if (st == DCS_OK && tHost > 0 && tDev > 0)
    {
        if (tHost > tDev + 0.15 && ctx->sharedHostParts > 0)
            ctx->sharedHostParts -= 1;
        else if (tDev > tHost + 0.15 && ctx->sharedHostParts < static_cast<int>(kParts) - 1)
            ctx->sharedHostParts += 1;
    }
    if (pipeSwitches().trace)
        fprintf(stderr, "decode in parts: %u of %u parts walked by the host pool, done at %.2f ms; the device's at %.2f ms; next call %d\n",
                hostParts, kParts, tHost, tDev, ctx->sharedHostParts);
}

// dcs_decode_streams for a LARGE list: cut into parts (contiguous stream ranges balanced by frames) that go through a
// pipeline the context keeps for the purpose (index pass on the host pool), so that the planner, packer and upload of
// one part run while another part is indexed and a third decodes and comes back; every worker copies its part's PCM
// straight into the caller's buffer.  One synchronous call for the caller, the same PCM -- 15 ms become 5 for 65 536
// frames.  *handled = false: the list is small, the caller takes the direct path.
DcsStatus dcsDecodeStreamsInParts(DcsCtx *ctx, const DcsStreamRef *streams, uint32_t nStreams, uint32_t extraFrames,
                                  int16_t *pcmOut, size_t pcmCapFrames, uint32_t *frameOffsets, uint32_t *errOut, bool *handled)
{
    *handled = false;
    if (nStreams < 4 * kParts)
        return DCS_OK;
    std::vector<uint32_t> frames(nStreams);
    std::vector<uint64_t> first(static_cast<size_t>(nStreams) + 1, 0);
    for (uint32_t k = 0 ; k < nStreams ; ++k)
    {
        if (streams[k].data == nullptr || streams[k].len < 3)
            return DCS_OK;                          // (the direct path reports it)
        const uint32_t nf = (static_cast<uint32_t>(streams[k].data[0]) << 8) | streams[k].data[1];
        if (nf == 0)
            return DCS_OK;
        frames[k] = nf + extraFrames;
        first[k + 1] = first[k] + frames[k];
    }
    if (first[nStreams] < 32768 || first[nStreams] > pcmCapFrames || first[nStreams] > 0xFFFFFFFFull)
        return DCS_OK;
    const bool onDevice = ctx->largeListOnDevice;
    if (ctx->internalPipe == nullptr)
    {
        const DcsStatus st = pipelineCreate(ctx, static_cast<int>(kParts), (onDevice ? DCS_PIPE_ALL_ON_DEVICE : 0u) | kPipeLatency, &ctx->internalPipe);
        if (st != DCS_OK)
            return DCS_OK;                          // (no pipeline: the direct path still works)
        if (onDevice)
            ctx->internalPipe->roundGather = kParts;
    }
    DcsPipeline *const pipe = ctx->internalPipe;
    *handled = true;
    // The parts taper: the call ends one part's latency (build, create, upload, kernel, download) after the index pass
    // has reached the list's last stream, so the last parts are small -- 4 4 4 4 3 2 2 1 twenty-fourths of the frames
    // (equal parts: 4.6 ms for 65 536 frames, of which 1.45 behind the index pass).
    // (the walk shared with the device: the device walks the LAST part(s), and what it does behind its walk -- planner, packer,
    // decode, the PCM's way down -- is the call's tail: those parts are the small ones)
    static const uint32_t kWeightHost[kParts] = { 4, 4, 4, 4, 3, 2, 2, 1 }, kWeightDevice[kParts] = { 3, 3, 3, 3, 3, 3, 3, 3 },
                          kWeightShared[kParts] = { 4, 4, 4, 3, 3, 3, 2, 1 };
    uint32_t cut[kParts + 1];
    cutIntoParts(first, !onDevice ? kWeightHost : ctx->largeListShared ? kWeightShared : kWeightDevice, cut);
    DcsStatus st = DCS_OK;
    // the index pass over the WHOLE list in one region of the host pool (eight regions of 32 streams each would balance
    // badly over the pool's threads), then the parts go to the workers with their records
    // (only the host-index path needs them: 148 B per frame, kept per calling thread; the device path leaves them empty)
    thread_local std::vector<DcsFrameIndex> records;
    std::vector<DcsStreamInfo> infos;
    std::vector<uint64_t> firstRecord;
    // where the records of each of the first `count` streams, which the host pool walks, begin -> how many there are
    const auto recordStarts = [&](uint32_t count) {
        firstRecord.resize(count);
        uint64_t nRec = 0;
        for (uint32_t k = 0 ; k < count ; ++k)
        {
            firstRecord[k] = nRec;
            nRec += frames[k] - extraFrames;
        }
        return nRec;
    };
    // what the pool walks and where its records and stream summaries go (`records` is thread-local: the pool threads must not name it)
    uint32_t walkStreams = 0;
    DcsFrameIndex *walkRecs = nullptr;
    DcsStreamInfo *walkInfos = nullptr;
    if (!onDevice)
    {
        walkStreams = nStreams;
        infos.resize(nStreams);
        const uint64_t nRec = recordStarts(nStreams);
        if (records.size() < nRec)
            records.resize(nRec);
        walkRecs = records.data();
        walkInfos = infos.data();
    }
    const double tI0 = nowMs();
    // a part goes to the workers the moment the last of its streams has been indexed (by whichever pool thread that was):
    // planner, packer, upload and decode of the early parts run under the index pass of the late ones
    std::atomic<uint32_t> left[kParts];
    std::atomic<uint32_t> submitted{ 0 };
    std::atomic<int> submitError{ DCS_OK };
    std::vector<uint8_t> partOf(nStreams);
    for (uint32_t r = 0 ; r < kParts ; ++r)
    {
        left[r].store(cut[r + 1] - cut[r]);
        for (uint32_t k = cut[r] ; k < cut[r + 1] ; ++k)
            partOf[k] = static_cast<uint8_t>(r);
    }
    // part r to the pipeline, with the pool's records of it (or none: the device walks it); the first error is kept
    const auto submitPart = [&](uint32_t r, const DcsFrameIndex *recs, const uint64_t *firstRec, const DcsStreamInfo *infs) {
        const uint64_t f0 = first[cut[r]];
        const DcsStatus s1 = pipelineSubmit(pipe, streams + cut[r], cut[r + 1] - cut[r], extraFrames, pcmOut + f0 * DCS_FRAME_SAMPLES,
                                            errOut ? errOut + f0 : nullptr, recs, recs ? firstRec + cut[r] : nullptr, recs ? infs + cut[r] : nullptr);
        int expected = DCS_OK;
        if (s1 == DCS_OK)
            submitted.fetch_add(1);
        else
            submitError.compare_exchange_strong(expected, s1);
        return s1;
    };
    const int idxThreads = 0;        // (all of the pool: leaving a quarter of the CPUs to the workers was measured, 6.8 against 5.8 ms)
    CacheBuf sharedPinned;
    uint32_t hostParts = 0;
    double tCall0 = nowMs();
    if (onDevice)
    {
        // The walk SHARED between host and device (dcs_ctx_set_large_list_path 2, the default; round 5).  The index kernel takes as
        // long as its longest stream whatever the number of streams (a lone wavefront per stream: 1.9 ms for 256 frames), and until
        // it is through nothing of the list can be decoded; the host pool walks a stream fourteen times faster and delivers the
        // list's FIRST parts while the device walks the last ones: their planner, packer, decode and -- what counts -- their PCM's
        // way down run under the index kernel.  The host's records are the index kernel's, byte for byte (tests/test_gpu_parity.py),
        // so they go up and take its place (pipelineWorker).  How many parts the host takes follows what was measured: the side
        // that finished later in the last call gets less in the next.
        hostParts = ctx->largeListShared ? static_cast<uint32_t>(std::max(0, std::min(static_cast<int>(kParts) - 1, ctx->sharedHostParts))) : 0u;
        //  The pool runs ONE parallel region at a time: with several contexts decoding large lists at once (dcs_node,
        // dcs_decode_streams_sharded: a thread per device) the shared walks would queue up one behind the other, the last device
        // waiting (N - 1) host walks before its first part is even submitted.  A context that finds the pool taken walks its whole
        // list on its own device (mode 1's 3.3 ms, whatever the others do).  A share that has fallen to nothing is tried again
        // with one part every sixteenth call.
        if (hostParts != 0 && dcsIndexPoolBusy())
            hostParts = 0;
        if (ctx->largeListShared && ctx->sharedHostParts == 0 && (++ctx->sharedProbe & 15) == 0 && !dcsIndexPoolBusy())
            hostParts = 1;
        if (hostParts != 0)
        {
            const uint32_t hostStreams = cut[hostParts];
            const uint64_t hostRecs = recordStarts(hostStreams);
            if (sharedPinned.alloc(ctx, true, sizeof(DcsFrameIndex) * hostRecs + sizeof(DcsStreamInfo) * hostStreams + 64) != hipSuccess)
            {
                (void)hipGetLastError();
                hostParts = 0;
            }
            else
            {
                walkStreams = hostStreams;
                walkRecs = sharedPinned.as<DcsFrameIndex>();
                walkInfos = reinterpret_cast<DcsStreamInfo *>(sharedPinned.as<uint8_t>() + ((sizeof(DcsFrameIndex) * hostRecs + 15) & ~size_t(15)));
            }
        }
        {
            std::lock_guard<std::mutex> lk(pipe->m);
            pipe->roundGather = kParts - hostParts;           // (the index round waits until its parts are all there)
            pipe->lastHostWalkedDone = pipe->lastDeviceWalkedDone = 0;
        }
        tCall0 = nowMs();
        // the device's parts first: index walk, planner, packer and decode on the device, the workers copy the PCM out
        for (uint32_t r = hostParts ; r < kParts && st == DCS_OK ; ++r)
            st = submitPart(r, nullptr, nullptr, nullptr);
    }
    if (walkStreams != 0 && st == DCS_OK)
    {
        // ... and the host's: a part goes to the pipeline the moment the pool has walked the last of its streams
        const std::function<void(uint32_t)> walked = [&, walkRecs, walkInfos](uint32_t k) {
            const uint32_t r = partOf[k];
            if (left[r].fetch_sub(1) == 1)
                submitPart(r, walkRecs, firstRecord.data(), walkInfos);
        };
        st = dcsIndexStreamsNotify(streams, walkStreams, idxThreads, walkRecs, firstRecord.data(), walkInfos, nullptr, &walked);
        if (st == DCS_OK)
            st = static_cast<DcsStatus>(submitError.load());
    }
    const double tI1 = nowMs();
    for (uint32_t r = 0, n = submitted.load() ; r < n ; ++r)
    {
        DcsPipelineResult res;
        const DcsStatus s1 = dcs_pipeline_collect(pipe, &res);
        if (st == DCS_OK)
            st = s1;
    }
    if (onDevice && hostParts != 0)
        adjustSharedHostParts(ctx, st, tCall0, hostParts);
    sharedPinned.release();
    if (pipeSwitches().trace)
        fprintf(stderr, "decode in parts: index %.2f ms, parts %.2f ms\n", tI1 - tI0, nowMs() - tI1);
    if (frameOffsets != nullptr)
        for (uint32_t k = 0 ; k <= nStreams ; ++k)
            frameOffsets[k] = static_cast<uint32_t>(first[k]);
    return st;
}
