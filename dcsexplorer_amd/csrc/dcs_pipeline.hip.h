// dcs_pipeline.hip.h -- lists of streams in flight: the host preparation of one list (index pass, mixing parameters,
// chunk planner, packer) runs while the GPU decodes another and a third comes back into pinned memory.  Included at
// the end of dcs_runtime.hip (it uses the runtime's batch internals).
//
// The reference decodes its batch job (`--extract-streams`, DCSExplorer.cpp:1742-1907) one stream after the other on
// one thread; here a caller submits lists of whole streams and collects their PCM in submission order.
//
// Shapes, chosen at creation:
//   index pass on the host pool (default): `depth` worker threads each take a submitted list through all its stages on
//     a HIP stream of their own, so the stages of different lists overlap by themselves.
//   index pass on the device (DCS_PIPE_INDEX_ON_DEVICE): the index pass is most of a list's host work (tools/hostbench.cpp:
//     35 of 45 CPU-milliseconds for 65 536 frames), and the host has no cores to spare.  A worker uploads its list's streams
//     (stage A) and hands the list to an INDEXER thread, which walks the streams of the lists that are waiting -- one
//     wavefront per stream, dcs_index_wave.hip.h; a round of up to 2 048 streams takes 2.4 to 2.7 ms whatever their number,
//     every list's records go to buffers of its own -- copies the records back and passes the lists on; a worker then
//     builds, plans, packs, decodes and downloads (stage B).
//   ... and the packer on the device too (DCS_PIPE_PACK_ON_DEVICE): the records do not come back at all.  The indexer
//     copies back an 8-byte digest per frame (bit offset, bit count, band count, flags), the worker plans from that, and
//     a pack kernel assembles the packages from the records and streams that are already resident.
//   ... and the planner (DCS_PIPE_PLAN_ON_DEVICE): nothing of the index results comes back.  A list of whole streams has a
//     regular job list, so one thread per chunk works the chunk plan out (dcsPlanKernel); a worker queues planner, packer,
//     decode kernel and the copy down behind the indexers' round and sleeps until the PCM is there.  Lists the arithmetic
//     plan cannot serve are decoded by the host-planned path (DcsPipelineResult.path).
// The context keeps a pipeline of its own for dcs_decode_streams on a large list (dcsDecodeStreamsInParts, dcs_large_list.hip.h).
//
// Output, chosen at creation too: PCM (default), or FLAC (DCS_PIPE_FLAC, with DCS_PIPE_FLAC_MD5 the samples' MD5 in it): the writer
// (dcs_flac_held.h) is queued behind the batch's launch on the worker's stream, the FLAC bytes, their table and the error words come
// down into pinned memory the list keeps until it is collected, and the worker waits once.  The PCM never leaves the device.
//
// Stage B is made of steps that the host-planned path (pipelineDecode) and the device-planned one (pipelineDecodePlanned, up to
// three attempts) share: pipelinePrepare (host-planned only: where the records come from), pipelineLaunch (options, the batch, its
// run), pipelineBringDown (the ending, PCM or FLAC: the one place that knows there are two), and then either pipelineDeliver
// (into a caller's memory) or pipelineAbandon.  What a list holds is the Job's: Job::releaseInputs() gives back what the index
// pass and the packer read, Job::releaseResults() the batch and the FLAC buffers; the environment's switches are PipeSwitches.
#pragma once
#include "dcs_flac_held.h"
#include <condition_variable>
#include <deque>
#include <memory>
#include <thread>
#include <atomic>
#include <climits>
#include <pthread.h>

struct DcsPipeline
{
    struct BatchDeleter { void operator()(DcsBatch *b) const { dcs_batch_destroy(b); } };
    struct EventDeleter { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };

    // A list and everything it holds.  Nothing here waits, and the cache (which knows nothing of streams) hands a buffer that came
    // back to the next who asks: whoever lets go of something that work queued on a stream may still use waits for that stream first
    // (dcs_cache.h, dcs_flac_held.h), and the list's device is the current one.  A list that succeeded has waited for its PCM or FLAC,
    // which its stream delivers after everything else.
    struct Job
    {
        const DcsStreamRef *streams = nullptr;
        uint32_t nStreams = 0, extraFrames = 0;
        std::vector<uint32_t> firstJob;         // first output frame of each stream, and the total
        std::unique_ptr<DcsBatch, BatchDeleter> batch;
        const int16_t *pcm = nullptr;
        const uint32_t *err = nullptr;
        DcsStatus status = DCS_OK;
        bool done = false;
        double hostMs = 0, deviceMs = 0;        // wall time of the threads that worked on the list: host preparation /
                                                // uploads + kernels + downloads (the device index pass counts here)
        // ---- index pass on the device
        bool onDevice = false;                  // records came from the device; the streams lie in hBlob
        uint32_t path = 0;                      // DCS_PIPE_*: the stages of THIS list that ran on the device
        CacheBuf hBlob;                         // the streams as uploaded, end to end (pinned); the packer reads them
        size_t hBlobLen = 0;
        CacheBuf dBlob;                         // the same on the device, for the walk only
        std::vector<DcsStreamLoc> locs;         // offsets relative to the list's blob
        std::vector<uint64_t> firstRecord, streamOff;
        uint64_t totalRec = 0;
        CacheBuf hRec, hInfo;                   // records (or, packing on the device, their digests) and stream summaries
                                                //   as they come back (pinned)
        std::unique_ptr<std::remove_pointer<hipEvent_t>::type, EventDeleter> uploaded;
        // results copied into caller memory by the worker (dcs_decode_streams in parts): optional
        int16_t *pcmDst = nullptr;
        uint32_t *errDst = nullptr;
        // index records the submitter already has (host memory that outlives the job): the index pass is skipped
        const DcsFrameIndex *preRecords = nullptr;
        const uint64_t *preFirstRecord = nullptr;
        const DcsStreamInfo *preInfos = nullptr;
        double tSubmit = 0, tTaken = 0, tQueuedForIndex = 0, tIndexStart = 0, tIndexed = 0, tStageB = 0, tDone = 0;     // (DCS_PIPE_TRACE)
        // what the index round writes for this list (device; fixed sizes per list, so the context's cache serves them): the
        // records -- which stay resident for the device packer --, their digests, the stream summaries
        CacheBuf dRec, dDigest, dInfo;
        const DcsFrameIndex *dRecords = nullptr;    // = dRec once the round has run
        // ---- FLAC out: the writer's buffers and the error words' pinned copy, the list's until it is collected
        FlacHeld flac;
        CacheBuf hErrFlac;

        // The two releases, each in the order in which its buffers go back (not the members': the cache evicts what came back first).
        // What the index pass and the packer read: given back once the packages are on the device, or once the list is given up.
        void releaseInputs()
        {
            dRecords = nullptr;
            for (CacheBuf *c : { &dRec, &dDigest, &dInfo, &dBlob, &hRec, &hInfo, &hBlob })
                c->release();
            uploaded.reset();
        }
        // What the caller reads: given back when the next list is collected, or between the attempts of a list planned again.
        void releaseResults()
        {
            batch.reset();
            flac.release();
            hErrFlac.release();
            pcm = nullptr;
            err = nullptr;
        }
        ~Job() { releaseInputs(); releaseResults(); }      // (a backstop: every path through the pipeline has called both by now)
    };
    typedef std::shared_ptr<Job> JobPtr;

    DcsCtx *ctx = nullptr;
    int depth = 0;
    size_t roundGather = 0;                 // > 1: an index round waits (briefly) until so many lists are there
    uint32_t flags = 0;                             // DCS_PIPE_*
    std::mutex m;
    std::condition_variable work, indexWork, finished, room;
    std::deque<JobPtr> fresh;                       // submitted, not yet taken by a worker
    std::deque<JobPtr> toIndex;                     // uploaded, waiting for the indexer
    std::deque<JobPtr> indexed;                     // records are back: ready for stage B
    std::deque<JobPtr> order;                       // submitted, not yet collected (submission order)
    JobPtr held;                                    // the list whose result the caller is reading
    std::vector<std::thread> workers;
    std::vector<std::thread> indexers;
    int nWorkers = 0, nUploaders = 0;               // (device index pass: the first nUploaders workers do stage A only)
    std::vector<hipStream_t> streams;               // one per worker, and one more for each indexer
    bool quit = false;
    // dcsDecodeStreamsInParts with the walk shared between host and device: when the last list of either kind was finished
    double lastHostWalkedDone = 0, lastDeviceWalkedDone = 0;
};

static double nowMs()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// internal flag: the pipeline's threads wait by polling inside the runtime (shortest latency) instead of napping
static constexpr uint32_t kPipeLatency = 0x100u;

// The environment's switches, read ONCE, with the first pipeline of the process (or the first batch made as a pipeline makes them).
// Experiment switches all: 0 or null means "not set", and the rule next to the use holds.
struct PipeSwitches
{
    int trace = 0;                  // DCS_PIPE_TRACE: set at all, a line or two per list; 2, what every thread did and when; 3, stage B waits
                                    //   for its kernels before the copies
    unsigned upBlocks = 0;          // DCS_PIPE_UP_BLOCKS: workgroups of a list's upload
    int downBlocks = 0;             // DCS_PIPE_DOWN_BLOCKS: the PCM comes down by copy kernel, with at most so many workgroups
    size_t roundStreams = 0;        // DCS_PIPE_ROUND_STREAMS: the most streams an index round takes
    int workers = 0, uploaders = 0; // DCS_PIPE_WORKERS (1 to 64; stage-B workers where there are uploaders), DCS_PIPE_UPLOADERS (1 to 8)
    char indexerPrio[2] = { 0, 0 }; // DCS_PIPE_INDEXER_PRIO=ab, a / b one of l(east) g(reatest) n(ormal): the two indexers' stream priorities
    bool xcdRanges = true;          // DCS_PIPE_XCD_RANGES=0: the pipelines' batches are made without XCD ranges
};

static const PipeSwitches &pipeSwitches()
{
    static const PipeSwitches switches = [] {
        PipeSwitches s;
        const auto number = [](const char *name, int lo, int hi, int unset) {
            const char *e = getenv(name);
            return e == nullptr ? unset : std::max(lo, std::min(hi, atoi(e)));
        };
        s.trace = number("DCS_PIPE_TRACE", 1, INT_MAX, 0);
        s.upBlocks = static_cast<unsigned>(number("DCS_PIPE_UP_BLOCKS", 1, INT_MAX, 0));
        s.downBlocks = number("DCS_PIPE_DOWN_BLOCKS", INT_MIN, INT_MAX, 0);
        s.roundStreams = static_cast<size_t>(number("DCS_PIPE_ROUND_STREAMS", 1, INT_MAX, 0));
        s.workers = number("DCS_PIPE_WORKERS", 1, 64, 0);
        s.uploaders = number("DCS_PIPE_UPLOADERS", 1, 8, 0);
        if (const char *e = getenv("DCS_PIPE_INDEXER_PRIO"))
        {
            s.indexerPrio[0] = e[0];
            s.indexerPrio[1] = e[0] ? e[1] : 0;
        }
        s.xcdRanges = number("DCS_PIPE_XCD_RANGES", INT_MIN, INT_MAX, 1) != 0;
        return s;
    }();
    return switches;
}

// DCS_PIPE_TRACE=2: what every pipeline thread did and when (tools/pipe_threads.py reads it from stderr)
static void pipeLog(const char *who, int id, const char *what, double t0, double t1, size_t q1 = 0, size_t q2 = 0)
{
    if (pipeSwitches().trace >= 2)
        fprintf(stderr, "pipe thread: %s %d %s %.3f %.3f %zu %zu\n", who, id, what, t0, t1, q1, q2);
}

// the list a caller has read, or one that was never collected, goes (the caller has set the device)
static void pipelineRelease(DcsPipeline::JobPtr &job)
{
    if (job)
    {
        job->releaseInputs();
        job->releaseResults();
    }
    job.reset();
}

static void pipelineFinish(DcsPipeline *p, const DcsPipeline::JobPtr &job, DcsStatus st)
{
    {
        std::lock_guard<std::mutex> lk(p->m);
        job->status = st;
        job->done = true;
        (job->preRecords != nullptr ? p->lastHostWalkedDone : p->lastDeviceWalkedDone) = nowMs();
    }
    p->finished.notify_all();
}

// The streams of a list end to end, each on a 4-byte boundary and no longer than its header plus nFrames maximal frames (the
// caller's buffer may be the rest of a ROM): where each lies in the list's blob and where its index records go.
static DcsStatus layoutStreams(const DcsStreamRef *streams, uint32_t n, std::vector<DcsStreamLoc> &locs, std::vector<uint64_t> &firstRecord,
                              size_t *blobLenOut, uint64_t *totalRecOut)
{
    locs.resize(n); firstRecord.resize(n);
    size_t blobLen = 0;
    uint64_t totalRec = 0;
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const DcsStreamRef &sr = streams[k];
        if (sr.data == nullptr || sr.len < 3 || sr.os < DCS_OS93A || sr.os > DCS_OS95)
            return DCS_ERR_INVALID_ARG;
        const uint32_t nFrames = (static_cast<uint32_t>(sr.data[0]) << 8) | sr.data[1];
        if (nFrames == 0)
            return DCS_ERR_BAD_STREAM;
        const size_t most = 2 + 16 + (static_cast<size_t>(nFrames) * DCS_MAX_FRAME_BITS + 7) / 8 + 8;
        const size_t len = sr.len < most ? sr.len : most;
        blobLen = (blobLen + 3) & ~size_t(3);
        locs[k].off = blobLen; locs[k].len = static_cast<uint32_t>(len); locs[k].os = sr.os; locs[k].firstRecord = totalRec;
        firstRecord[k] = totalRec;
        blobLen += len;
        totalRec += nFrames;
    }
    *blobLenOut = blobLen;
    *totalRecOut = totalRec;
    return DCS_OK;
}

// stage A (device index pass): lay the list's streams end to end in pinned memory and send them up
static DcsStatus pipelineUpload(DcsPipeline *p, DcsPipeline::Job *job, hipStream_t stream)
{
    DcsCtx *ctx = p->ctx;
    const uint32_t n = job->nStreams;
    {
        const DcsStatus st = layoutStreams(job->streams, n, job->locs, job->firstRecord, &job->hBlobLen, &job->totalRec);
        if (st != DCS_OK)
            return st;
    }
    job->streamOff.resize(n);
    for (uint32_t k = 0 ; k < n ; ++k)
        job->streamOff[k] = job->locs[k].off;
    const size_t blobLen = job->hBlobLen, blobBytes = deviceBlobBytes(blobLen);
    const uint64_t totalRec = job->totalRec;
    const double tu0 = nowMs();
    HIPCHK(ctx, job->hBlob.alloc(ctx, true, blobBytes));
    const bool planOnDevice = (p->flags & DCS_PIPE_PLAN_ON_DEVICE) != 0;       // (then nothing of the index pass comes back to the host)
    if (!planOnDevice)
    {
        HIPCHK(ctx, job->hRec.alloc(ctx, true, ((p->flags & DCS_PIPE_PACK_ON_DEVICE) ? sizeof(DcsFrameDigest) : sizeof(DcsFrameIndex)) * totalRec));
        HIPCHK(ctx, job->hInfo.alloc(ctx, true, sizeof(DcsStreamInfo) * n));
    }
    HIPCHK(ctx, job->dBlob.alloc(ctx, false, blobBytes));
    HIPCHK(ctx, job->dRec.alloc(ctx, false, sizeof(DcsFrameIndex) * (totalRec ? totalRec : 1)));
    if ((p->flags & DCS_PIPE_PACK_ON_DEVICE) && !planOnDevice)
        HIPCHK(ctx, job->dDigest.alloc(ctx, false, sizeof(DcsFrameDigest) * (totalRec ? totalRec : 1)));
    HIPCHK(ctx, job->dInfo.alloc(ctx, false, sizeof(DcsStreamInfo) * n));
    const double tu1 = nowMs();
    uint8_t *hBlob = job->hBlob.as<uint8_t>();
    memset(hBlob + blobLen, 0, blobBytes - blobLen);
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const DcsStreamLoc &l = job->locs[k];
        if (k + 1 < n)          // (the alignment gap in front of the next stream)
            memset(hBlob + l.off + l.len, 0, static_cast<size_t>(job->locs[k + 1].off - l.off) - l.len);
        memcpy(hBlob + l.off, job->streams[k].data, l.len);
    }
    const double tu2 = nowMs();
    hipEvent_t uploaded = nullptr;
    HIPCHK(ctx, hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
    job->uploaded.reset(uploaded);
    // The streams go up through EIGHT workgroups (DCS_PIPE_UP_BLOCKS overrides).  A copy kernel that reads pinned host memory with hundreds of
    // workgroups -- 2.4 MB a list: 586 of them -- keeps that many wavefronts stalled on PCIe reads whose completions travel the
    // direction the PCM's writes need: the PCM of the lists further along came down at 70-75 % of the link's rate.  With 4 to 20
    // workgroups (an upload then takes 0.15 ms instead of 0.05) the link runs at 93-97 %: 0.74 -> 0.58 ms per list sustained (round 4).
    // (a list far larger than those measured gets more of them, one per 300 KB up to 32, so that its upload stays shorter than its PCM's way down)
    const unsigned upBlocksEnv = pipeSwitches().upBlocks;
    const unsigned upBlocks = upBlocksEnv != 0 ? upBlocksEnv : static_cast<unsigned>(std::min<size_t>(32, std::max<size_t>(8, blobBytes / (300u << 10))));
    HIPCHK(ctx, copyByKernel(stream, job->dBlob.as(), hBlob, blobBytes, (p->flags & kPipeLatency) ? 1024u : upBlocks));
    HIPCHK(ctx, hipEventRecord(uploaded, stream));
    if (pipeSwitches().trace)
        fprintf(stderr, "pipe upload: allocs %.2f, memcpy %.2f, hip calls %.2f\n", tu1 - tu0, tu2 - tu1, nowMs() - tu2);
    return DCS_OK;
}

// the indexer: ONE launch of the index kernel over the streams of every list that is waiting
static void pipelineIndexer(DcsPipeline *p, int which)
{
    pthread_setname_np(pthread_self(), "dcs-indexer");
    tlsBlockingWaits = (p->flags & kPipeLatency) == 0;      // (the context's own pipeline serves ONE waiting caller: its threads poll)
    DcsCtx *ctx = p->ctx;
    (void)hipSetDevice(ctx->device);
    const hipStream_t stream = p->streams[static_cast<size_t>(p->nWorkers + which)];
    // A round takes the lists that are waiting, up to about an eighth of the chip's wavefront slots (one wavefront walks one
    // stream, for milliseconds): the decode kernels of the lists further along must find room next to it, and beyond that
    // size a round's time grows with its streams anyway (2 048 streams x 256 frames 2.7 ms, 8 192 6.0 ms).
    const size_t maxRoundStreams = pipeSwitches().roundStreams != 0 ? pipeSwitches().roundStreams : static_cast<size_t>(ctx->numCUs) * 8;
    GrowBuf hTable(true), dTable;       // the round's stream locations and result addresses, as uploaded; freed when the thread ends
    for (;;)
    {
        std::vector<DcsPipeline::JobPtr> jobs;
        {
            std::unique_lock<std::mutex> lk(p->m);
            p->indexWork.wait(lk, [&] { return p->quit || !p->toIndex.empty(); });
            // (a caller that submits the parts of ONE list wants them in one round: wait a moment for the rest)
            if (p->roundGather > 1 && !p->quit)
                p->indexWork.wait_for(lk, std::chrono::microseconds(400), [&] { return p->quit || p->toIndex.size() >= p->roundGather; });
            if (p->quit && p->toIndex.empty())
                return;
            size_t roundStreams = 0;
            while (!p->toIndex.empty() && (jobs.empty() || roundStreams + p->toIndex.front()->nStreams <= maxRoundStreams))
            {
                roundStreams += p->toIndex.front()->nStreams;
                jobs.push_back(p->toIndex.front());
                p->toIndex.pop_front();
            }
        }
        if (jobs.empty())       // (the other indexer took every list while this one dropped the mutex in the gather wait)
            continue;
        const double t0 = nowMs();
        for (const DcsPipeline::JobPtr &j : jobs) j->tIndexStart = t0;
        // stream locations with ABSOLUTE device addresses (the kernel's blob base is address 0); every list's results go to
        // buffers of its own, so a round allocates nothing but its table of locations (kept from round to round)
        uint32_t nStreams = 0;
        for (const DcsPipeline::JobPtr &j : jobs) nStreams += j->nStreams;
        const size_t locBytes = sizeof(DcsStreamLoc) * nStreams, tableBytes = locBytes + sizeof(dcsidx::StreamOut) * nStreams;
        const bool packOnDevice = (p->flags & DCS_PIPE_PACK_ON_DEVICE) != 0;
        DcsStatus st = [&]() -> DcsStatus {
            if (std::min(hTable.capacity(), dTable.capacity()) < tableBytes)        // (twice what the round needs, for the rounds to come)
            {
                HIPCHK(ctx, hTable.room(tableBytes * 2));
                HIPCHK(ctx, dTable.room(tableBytes * 2));
            }
            DcsStreamLoc *locs = hTable.as<DcsStreamLoc>();
            dcsidx::StreamOut *outs = reinterpret_cast<dcsidx::StreamOut *>(hTable.as<uint8_t>() + locBytes);
            uint32_t k = 0;
            for (const DcsPipeline::JobPtr &j : jobs)
                for (uint32_t i = 0 ; i < j->nStreams ; ++i, ++k)
                {
                    const DcsStreamLoc &l = j->locs[i];
                    locs[k] = l;
                    locs[k].off = reinterpret_cast<uint64_t>(j->dBlob.as()) + l.off;
                    outs[k].records = j->dRec.as<DcsFrameIndex>() + l.firstRecord;
                    outs[k].digest = j->dDigest ? j->dDigest.as<DcsFrameDigest>() + l.firstRecord : nullptr;
                    outs[k].info = j->dInfo.as<DcsStreamInfo>() + i;
                }
            for (const DcsPipeline::JobPtr &j : jobs)
                HIPCHK(ctx, hipStreamWaitEvent(stream, j->uploaded.get(), 0));
            HIPCHK(ctx, copyByKernel(stream, dTable.as(), hTable.as(), tableBytes));
            HIPCHK(ctx, launchIndexWave(stream, 0, dTable.as<const DcsStreamLoc>(), nStreams, ctx->dTables, nullptr, nullptr, nullptr,
                                        reinterpret_cast<const dcsidx::StreamOut *>(dTable.as<const uint8_t>() + locBytes)));
            for (const DcsPipeline::JobPtr &j : jobs)
                if (j->hRec)                    // (planner on the device: the records stay where they are)
                {
                    HIPCHK(ctx, hipMemcpyAsync(j->hRec.as(), (packOnDevice ? j->dDigest : j->dRec).as(), j->hRec.bytes(), hipMemcpyDeviceToHost, stream));
                    HIPCHK(ctx, hipMemcpyAsync(j->hInfo.as(), j->dInfo.as(), j->hInfo.bytes(), hipMemcpyDeviceToHost, stream));
                }
            HIPCHK(ctx, streamWait(ctx, stream));
            return DCS_OK;
        }();
        if (st != DCS_OK)
            (void)streamWait(ctx, stream);
        if (packOnDevice && st == DCS_OK)
            for (const DcsPipeline::JobPtr &j : jobs)
                j->dRecords = j->dRec.as<const DcsFrameIndex>();      // (they stay until the list has packed)
        const double dt = nowMs() - t0;
        pipeLog("indexer", which, "round", t0, nowMs(), jobs.size(), nStreams);
        {
            std::lock_guard<std::mutex> lk(p->m);
            for (const DcsPipeline::JobPtr &j : jobs)
            {
                j->deviceMs += dt;
                j->status = st;
                j->tIndexed = nowMs();
                p->indexed.push_back(j);
            }
        }
        p->work.notify_all();
    }
}

// Why a pipeline's batches are launched in XCD ranges (DCS_BATCH_XCD_RANGES, dcs_common.h).  A decode kernel's wavefronts may wait
// for a tail another of ITS wavefronts publishes (dcs_kernels.hip.h: hand-off).  Workgroups are dispatched in index order and a
// producer lies in a lower-numbered chunk, so within ONE kernel that has the chip to itself every wait is for a wavefront that is
// resident or through.  Two such kernels side by side break that: workgroups go round-robin to the eight XCDs, each XCD fills its
// places on its own, and an XCD can be full of kernel B's waiting consumers whose producers sit undispatched on another XCD that is
// full of kernel A's waiting consumers -- whose producers wait for a place on the first.  Nothing moves until the bound of the wait
// (500 ms) flags the frames and the lists are decoded again: seen in round 4 as two lists in a hundred of 608 011 frames (76 000
// chunks each) and once in 400 lists of 65 536; short of that, the kernels of lists in flight held each other up for most of a
// millisecond (0.94 ms per decode kernel in the pipeline against 0.05 alone).  With chain order and XCD ranges a consumer's producer
// is dispatched before it on the consumer's own XCD, so no wait depends on a place becoming free.  (ONE decode stream per device,
// which also rules the circle out, was measured first: 0.92 ms per list instead of 0.60 -- lists waiting behind each other's packers.)

// (DCS_PIPE_XCD_RANGES=0, an experiment switch: the pipelines' batches are made without them)
static bool pipeXcdRanges() { return pipeSwitches().xcdRanges; }

// How a list's PCM comes down: by the runtime's copy (hipMemcpyAsync into pinned memory, which this runtime does with a blit
// kernel of its own), or -- DCS_PIPE_DOWN_BLOCKS=n, and always for a pipeline with ONE waiting caller (the context's own), where
// hipMemcpyAsync now and then holds the calling thread for 7 ms (profiles/NOTES.md 17) -- by dcsCopyKernel with at most n workgroups.
// Measured in round 4 (NOTES 24): with the uploads throttled (pipelineUpload) both ways down run at 93-97 % of the link.
static void pipelineDownPolicy(const DcsPipeline *p, DcsBatch *b)
{
    const int downBlocksEnv = pipeSwitches().downBlocks;
    const bool latency = (p->flags & kPipeLatency) != 0;
    b->downByKernel = latency || downBlocksEnv > 0;
    b->downBlocks = latency ? 1024u : static_cast<unsigned>(std::max(1, downBlocksEnv));
}

// The FLAC ending of stage B (DCS_PIPE_FLAC), in place of dcs_batch_download_view: the writer queued behind the batch's launch,
// the error words' copy behind it, ONE wait.  job->firstJob has the streams' first frames whatever planned the list.  The batch
// (its dPcm) outlives the wait.
static DcsStatus pipelineFlacDown(DcsPipeline *p, DcsPipeline::Job *job)
{
    DcsCtx *ctx = p->ctx;
    DcsBatch *b = job->batch.get();
    const uint32_t n = job->nStreams;
    if (job->firstJob.size() != static_cast<size_t>(n) + 1)
        return DCS_ERR_INVALID_ARG;
    thread_local std::vector<uint64_t> sampleOffsets;
    dcsFlacSampleOffsets(job->firstJob.data(), n, sampleOffsets);
    pipelineDownPolicy(p, b);
    const unsigned blocks = b->downByKernel ? b->downBlocks : 1024u;
    const size_t errBytes = sizeof(uint32_t) * b->nJobs;
    if (b->launched)
        HIPCHK(ctx, hipStreamWaitEvent(b->stream, b->evDone, 0));
    const DcsStatus st = dcsFlacWriteQueue(ctx, b->stream, b->dPcm.as<const int16_t>(), sampleOffsets.data(), n, 31250,
                                           (p->flags & DCS_PIPE_FLAC_MD5) ? DCS_FLAC_MD5 : 0u, job->flac, blocks);
    if (st != DCS_OK)
        return st;
    HIPCHK(ctx, job->hErrFlac.alloc(ctx, true, errBytes));
    HIPCHK(ctx, copyByKernel(b->stream, job->hErrFlac.as(), b->dErr, errBytes, 64u));
    HIPCHK(ctx, streamWait(ctx, b->stream));
    b->settled = true;
    job->pcm = nullptr;
    job->err = job->hErrFlac.as<const uint32_t>();
    return DCS_OK;
}

// ---- stage B's steps, shared by the host-planned and the device-planned path

// Launch: a batch as the pipelines make them (XCD ranges, see above) from whatever `create` has planned, and its run queued on the
// worker's stream.  *tCreated: when the batch was there (host work before, device work behind).
template <class Create>
static DcsStatus pipelineLaunch(DcsPipeline *p, DcsPipeline::Job *job, hipStream_t stream, double *tCreated, Create &&create)
{
    BatchOptions o(p->ctx, stream);
    o.xcdRanges = pipeXcdRanges();
    DcsBatch *b = nullptr;
    DcsStatus st = create(o, &b);
    job->batch.reset(b);
    *tCreated = nowMs();
    if (st == DCS_OK) st = dcs_batch_run(b, nullptr);
    return st;
}

// Bring down: the ending, with its one wait -- the PCM into the batch's pinned memory, or the FLAC written from it into the list's.
// The only place that knows there are two kinds of output.
static DcsStatus pipelineBringDown(DcsPipeline *p, DcsPipeline::Job *job)
{
    if ((p->flags & DCS_PIPE_FLAC) != 0)
        return pipelineFlacDown(p, job);
    pipelineDownPolicy(p, job->batch.get());
    return dcs_batch_download_view(job->batch.get(), &job->pcm, &job->err);
}

// Abandon: a list that failed, or that the device planner could not serve, may have left kernels in flight that read its inputs
// (the pack kernel reads dBlob and the round's records) and write its results: the batch goes (it waits for what it launched), the
// worker's stream is waited for, and then nothing of the attempt stays.
static void pipelineAbandon(DcsPipeline *p, DcsPipeline::Job *job, hipStream_t stream)
{
    job->batch.reset();
    (void)streamWait(p->ctx, stream);
    job->releaseResults();
    job->releaseInputs();
}

// Deliver: the results copied into caller memory by the worker (dcs_decode_streams in parts)
static void pipelineDeliver(DcsPipeline::Job *job, size_t nFrames)
{
    if (job->pcmDst == nullptr || job->pcm == nullptr)
        return;
    memcpy(job->pcmDst, job->pcm, sizeof(int16_t) * DCS_FRAME_SAMPLES * nFrames);
    if (job->errDst != nullptr)
        memcpy(job->errDst, job->err, sizeof(uint32_t) * nFrames);
}

// Prepare (host-planned path): where the list's index records come from, in this order of preference, and the plan made from them
enum PlanSource
{
    kPlanFromDigests,       // digests back from the device: the plan is in `planned`, the packer runs on the device
    kPlanFromRecords,       // records back from the device: `built`, over the streams as uploaded (hBlob)
    kPlanFromHost           // the submitter's records, or the host index pass: `built`, with a blob of its own
};

static DcsStatus pipelinePrepare(DcsPipeline *p, DcsPipeline::Job *job, DcsBuiltStreams &built, DcsBuiltPlan &planned, PlanSource *source)
{
    *source = kPlanFromHost;
    if (job->hRec)
    {
        // a stream whose frames run past its buffer reads the missing bytes as zero, which streams laid end to end
        // cannot express: such a list (truncated input) takes the host path.  What counts is the bits the frames
        // occupy, not nBytes, which includes the reference reader's look-ahead of up to three bytes (:1509).
        const DcsStreamInfo *infos = job->hInfo.as<const DcsStreamInfo>();
        bool fromDevice = true;
        for (uint32_t k = 0 ; k < job->nStreams && fromDevice ; ++k)
            fromDevice = infos[k].nFrames != 0
                      && 2u + static_cast<size_t>(infos[k].hdrLen) + (static_cast<size_t>(infos[k].payloadBits) + 7) / 8 <= job->locs[k].len;
        if (fromDevice && (p->flags & DCS_PIPE_PACK_ON_DEVICE) != 0 && job->dRecords != nullptr)
        {
            *source = kPlanFromDigests;
            const DcsDigested in{ job->hRec.as<const DcsFrameDigest>(), job->firstRecord.data(), infos, job->streamOff.data(), 0 };
            return dcsBuildPlanFromDigest(job->streams, job->nStreams, job->extraFrames, in, planned);
        }
        if (fromDevice)
        {
            *source = kPlanFromRecords;
            const DcsPreIndexed pre{ job->hRec.as<const DcsFrameIndex>(), job->firstRecord.data(), infos, job->streamOff.data() };
            return dcsBuildStreams(job->streams, job->nStreams, job->extraFrames, built, false, false, &pre);
        }
    }
    if (job->preRecords != nullptr)
    {
        const DcsPreIndexed pre{ job->preRecords, job->preFirstRecord, job->preInfos, nullptr };
        return dcsBuildStreams(job->streams, job->nStreams, job->extraFrames, built, false, false, &pre);
    }
    return dcsBuildStreams(job->streams, job->nStreams, job->extraFrames, built, false, false);
}

// stage B, planned on the host: from index records (device path) or from scratch (host pool) to PCM or FLAC in pinned memory
static DcsStatus pipelineDecode(DcsPipeline *p, DcsPipeline::Job *job, hipStream_t stream, int id)
{
    const double t0 = nowMs();
    // the batch description is needed only until the batch exists: one per worker thread, its memory kept from list to
    // list (fresh multi-megabyte vectors for every list cost more in page faults than everything else the host does)
    thread_local DcsBuiltStreams built;
    thread_local DcsBuiltPlan planned;
    PlanSource source;
    DcsStatus st = pipelinePrepare(p, job, built, planned, &source);
    const bool fromDevice = source != kPlanFromHost, devicePacked = source == kPlanFromDigests;
    job->onDevice = fromDevice;
    job->path = fromDevice ? (DCS_PIPE_INDEX_ON_DEVICE | (devicePacked ? DCS_PIPE_PACK_ON_DEVICE : 0u)) : 0u;
    job->firstJob = devicePacked ? planned.firstJob : built.firstJob;
    const size_t nJobs = devicePacked ? planned.jobs.size() : built.jobs.size();
    double t1 = nowMs(), t2 = t1;
    if (st == DCS_OK)
    {
        st = pipelineLaunch(p, job, stream, &t2, [&](const BatchOptions &o, DcsBatch **out) {
            if (devicePacked)
                return createBatchOnDevice(p->ctx, o, planned.jobs.data(), static_cast<uint32_t>(nJobs), planned.srcs.data(),
                                           static_cast<uint32_t>(planned.srcs.size()), job->dRecords, job->dBlob.as<const uint8_t>(),
                                           job->hBlobLen, out);
            return createBatch(p->ctx, o, fromDevice ? job->hBlob.as<const uint8_t>() : built.blob.data(), fromDevice ? job->hBlobLen : built.blob.size(),
                               built.srcs.data(), nullptr, static_cast<uint32_t>(built.srcs.size()), built.jobs.data(), static_cast<uint32_t>(nJobs), nullptr, 0, out);
        });
        // (DCS_PIPE_TRACE=3 waits for the kernels first, so that the thread log tells them from the copies)
        const double tk0 = nowMs();
        if (st == DCS_OK && pipeSwitches().trace >= 3) st = dcs_batch_sync(job->batch.get());
        const double tk1 = nowMs();
        if (st == DCS_OK) st = pipelineBringDown(p, job);
        pipeLog("worker", id, "kernels", tk0, tk1);
        pipeLog("worker", id, "download", tk1, nowMs());
    }
    if (st != DCS_OK)
        pipelineAbandon(p, job, stream);
    else
    {
        job->releaseInputs();           // (the packages are on the device: the streams are no longer needed)
        pipelineDeliver(job, nJobs);
    }
    const double t3 = nowMs();
    if (pipeSwitches().trace)
        fprintf(stderr, "pipe list: upload %.2f ms, index launch %.2f ms (records from the %s) | build %.2f create %.2f run+download %.2f\n",
                job->hostMs, job->deviceMs, fromDevice ? "device" : "host pool", t1 - t0, t2 - t1, t3 - t2);
    job->hostMs += t2 - t0;
    job->deviceMs += t3 - t2;
    return st;
}

// Planner on the device (DCS_PIPE_PLAN_ON_DEVICE), stage B: the list's index records are on the device (an indexer's round
// put them there); planner, packer and decode kernels and the PCM's way down are queued on the worker's stream, and the one
// wait is for the PCM.  Returns DCS_OK with *served = false when the arithmetic plan cannot serve the list (DCS_PLAN_*):
// the caller then takes the host-planned path.
static DcsStatus pipelineDecodePlanned(DcsPipeline *p, DcsPipeline::Job *job, hipStream_t stream, int id, bool *served)
{
    DcsCtx *ctx = p->ctx;
    *served = false;
    const double t0 = nowMs();
    // what the host knows of every stream without walking it
    thread_local DcsPlanTable table;
    DcsStatus st = planTableFor(job->streams, job->nStreams, job->extraFrames, job->locs.data(), job->firstRecord.data(), job->totalRec, table, job->firstJob);
    if (st != DCS_OK)
        return st;
    // A chunk whose frames' compressed bytes overflow the kernel's bit pool (224 bytes per slot) is what the arithmetic plan cannot
    // close early as the host planner does: the list is planned again with fewer frames per chunk -- three quarters, then half of the
    // slots -- before the host path gets it (one stream of large frames among 600 would otherwise cost the whole list the device).
    double t1 = t0, t2 = t0;
    uint32_t flag = 0;
    const int fullFpw = chooseFpw(ctx, static_cast<uint32_t>(table.nJobs), table.all94);
    const int tries[3] = { 0, fullFpw * 3 / 4, fullFpw / 2 };
    for (int attempt = 0 ; attempt < 3 ; ++attempt)
    {
        job->releaseResults();          // (an attempt before this one was waited for: what it queued is through)
        st = pipelineLaunch(p, job, stream, &t1, [&](const BatchOptions &o, DcsBatch **out) {
            return createBatchPlannedOnDevice(ctx, o, table, job->extraFrames, static_cast<uint32_t>(job->totalRec), job->dRec.as<const DcsFrameIndex>(),
                                              job->dInfo.as<const DcsStreamInfo>(), job->dBlob.as<const uint8_t>(), job->hBlobLen, out, tries[attempt]);
        });
        t2 = nowMs();
        pipeLog("worker", id, "plan-queue", t0, t1);
        pipeLog("worker", id, "run-queue", t1, t2);
        if (st == DCS_OK) st = pipelineBringDown(p, job);
        pipeLog("worker", id, "download", t2, nowMs());
        flag = st == DCS_OK ? batchPlanFlag(job->batch.get()) : 0;
        // again with fewer slots only for an overflow, and not when the list is (also) truncated: that one is the host's whatever the plan
        if (st != DCS_OK || (flag & DCS_PLAN_POOL_OVERFLOW) == 0 || (flag & DCS_PLAN_TRUNCATED) != 0)
            break;
    }
    job->hostMs += t1 - t0;
    job->deviceMs += nowMs() - t1;
    if (st != DCS_OK || flag != 0)
    {
        pipelineAbandon(p, job, stream);        // not served (or failed): nothing of this attempt stays
        return st;
    }
    job->onDevice = true;
    job->path = DCS_PIPE_INDEX_ON_DEVICE | DCS_PIPE_PACK_ON_DEVICE | DCS_PIPE_PLAN_ON_DEVICE;
    job->releaseInputs();
    pipelineDeliver(job, table.nJobs);
    *served = true;
    return DCS_OK;
}

static void pipelineWorker(DcsPipeline *p, int id)
{
    pthread_setname_np(pthread_self(), "dcs-worker");
    tlsBlockingWaits = (p->flags & kPipeLatency) == 0;      // (the context's own pipeline serves ONE waiting caller: its threads poll)
    (void)hipSetDevice(p->ctx->device);
    const hipStream_t stream = p->streams[id];
    const bool deviceIndex = (p->flags & DCS_PIPE_INDEX_ON_DEVICE) != 0;
    for (;;)
    {
        DcsPipeline::JobPtr job;
        bool stageB = false;
        {
            // With the index pass on the device the first `nUploaders` workers take ONLY fresh lists (stage A: lay the streams
            // out, send them up) and the others only indexed ones (stage B, which ends in a wait of milliseconds for the PCM).
            // When every worker took whatever was there, indexed lists first, the pipeline fell into lock step: all lists in
            // flight reached stage B together, the fresh ones behind them waited 20 ms for a worker, the indexers ran dry and
            // then walked everything in a burst (round 4, DCS_PIPE_TRACE=2: rounds of 8 lists back to back, then 20 ms of nothing).
            const bool takesFresh = !deviceIndex || id < p->nUploaders, takesIndexed = !deviceIndex || id >= p->nUploaders;
            std::unique_lock<std::mutex> lk(p->m);
            p->work.wait(lk, [&] { return p->quit || (takesIndexed && !p->indexed.empty()) || (takesFresh && !p->fresh.empty()); });
            if (takesIndexed && !p->indexed.empty())            // lists that are further along come first
            {
                job = p->indexed.front(); p->indexed.pop_front();
                stageB = true;
            }
            else if (takesFresh && !p->fresh.empty())
            {
                job = p->fresh.front(); p->fresh.pop_front();
            }
            else
                return;                         // quit
        }
        if (!stageB && deviceIndex)
        {
            const double t0 = nowMs();
            job->tTaken = t0;
            const DcsStatus st = pipelineUpload(p, job.get(), stream);
            job->hostMs += nowMs() - t0;
            pipeLog("worker", id, "upload", t0, nowMs());
            if (st != DCS_OK)
            {
                pipelineAbandon(p, job.get(), stream);
                pipelineFinish(p, job, st);
                continue;
            }
            if (job->preRecords != nullptr && (p->flags & DCS_PIPE_PLAN_ON_DEVICE))
            {
                // The host pool has walked this list already (dcsDecodeStreamsInParts, the walk shared with the device): its
                // records and stream summaries -- the very bytes the index kernel would have written -- go up behind the streams
                // and the list joins the indexed ones.  (Pinned memory of the caller's; this worker's stream is waited for, as an
                // indexer waits for its round, because stage B runs on another stream.)
                DcsStatus s2 = [&]() -> DcsStatus {
                    DcsCtx *ctx = p->ctx;
                    HIPCHK(ctx, copyByKernel(stream, job->dRec.as(), job->preRecords + job->preFirstRecord[0], sizeof(DcsFrameIndex) * job->totalRec, 64u));
                    HIPCHK(ctx, copyByKernel(stream, job->dInfo.as(), job->preInfos, job->dInfo.bytes(), 1u));
                    HIPCHK(ctx, streamWait(ctx, stream));
                    return DCS_OK;
                }();
                if (s2 != DCS_OK)
                    (void)streamWait(p->ctx, stream);
                const double t1 = nowMs();
                {
                    std::lock_guard<std::mutex> lk(p->m);
                    job->dRecords = job->dRec.as<const DcsFrameIndex>();
                    job->status = s2;
                    job->tQueuedForIndex = job->tIndexStart = job->tIndexed = t1;
                    p->indexed.push_back(job);
                }
                p->work.notify_all();
                continue;
            }
            {
                std::lock_guard<std::mutex> lk(p->m);
                job->tQueuedForIndex = nowMs();
                p->toIndex.push_back(job);
            }
            p->indexWork.notify_all();
            continue;
        }
        DcsStatus st = job->status;             // (the indexer's)
        job->tStageB = nowMs();
        if (st != DCS_OK)
        {
            // the index round failed (its thread has waited for its own stream; the streams' upload may not have been reached)
            if (job->uploaded) (void)hipEventSynchronize(job->uploaded.get());
            pipelineAbandon(p, job.get(), stream);
        }
        else
        {
            bool served = false;
            if (p->flags & DCS_PIPE_PLAN_ON_DEVICE)
            {
                st = pipelineDecodePlanned(p, job.get(), stream, id, &served);
                if (st == DCS_OK && !served)
                    pipeLog("worker", id, "not-served", job->tStageB, nowMs());
            }
            if (st == DCS_OK && !served)
                st = pipelineDecode(p, job.get(), stream, id);      // (host index pass, host planner: serves every list)
        }
        pipeLog("worker", id, "stageB", job->tStageB, nowMs());
        job->tDone = nowMs();
        if (pipeSwitches().trace && job->tIndexed != 0)
        {
            fprintf(stderr, "pipe life: submit->taken %.2f, upload %.2f, wait for indexer %.2f, index round %.2f, wait for worker %.2f, stage B %.2f\n",
                    job->tTaken - job->tSubmit, job->tQueuedForIndex - job->tTaken, job->tIndexStart - job->tQueuedForIndex,
                    job->tIndexed - job->tIndexStart, job->tStageB - job->tIndexed, job->tDone - job->tStageB);
        }
        pipelineFinish(p, job, st);
    }
}

static DcsStatus pipelineCreate(DcsCtx *ctx, int depth, uint32_t flags, DcsPipeline **out);

extern "C" DcsStatus dcs_pipeline_create(DcsCtx *ctx, int depth, uint32_t flags, DcsPipeline **out)
{
    if ((flags & ~(DCS_PIPE_INDEX_ON_DEVICE | DCS_PIPE_PACK_ON_DEVICE | DCS_PIPE_PLAN_ON_DEVICE | DCS_PIPE_FLAC | DCS_PIPE_FLAC_MD5)) != 0)
        return DCS_ERR_INVALID_ARG;
    if ((flags & DCS_PIPE_FLAC_MD5) != 0 && (flags & DCS_PIPE_FLAC) == 0)
        return DCS_ERR_INVALID_ARG;
    return pipelineCreate(ctx, depth, flags, out);
}

// (flags may carry kPipeLatency, which the public entry does not accept)
static DcsStatus pipelineCreate(DcsCtx *ctx, int depth, uint32_t flags, DcsPipeline **out)
{
    if (ctx == nullptr || out == nullptr || depth < 1 || depth > 64)
        return DCS_ERR_INVALID_ARG;
    if (flags & DCS_PIPE_PLAN_ON_DEVICE)
        flags |= DCS_PIPE_PACK_ON_DEVICE;
    if (flags & DCS_PIPE_PACK_ON_DEVICE)
        flags |= DCS_PIPE_INDEX_ON_DEVICE;           // (the packer works from the records the index pass leaves on the device)
    *out = nullptr;
    DcsPipeline *p = new (std::nothrow) DcsPipeline;
    if (p == nullptr)
        return DCS_ERR_NO_MEMORY;
    p->ctx = ctx;
    p->depth = depth;
    p->flags = flags;
    if (hipSetDevice(ctx->device) != hipSuccess)
    {
        delete p;
        setError(ctx, "dcs_pipeline_create: hipSetDevice failed");
        return DCS_ERR_HIP;
    }
    // with the index pass on the device a worker holds a list only while it works on it, so there need not be one per
    // list in flight: as many as the host has cores, and a few more for the ones that wait for a copy.  With the packer on
    // the device as well a list costs a worker under a millisecond of its own work, and what more workers add is contention
    // inside the HIP runtime: measured with 32 lists in flight on 16 CPUs, 4 to 6 workers 1.65-1.95 ms per list at 7-9 CPU-ms,
    // 10 workers 1.8-2.4, 20 workers 2.1-2.5 at 18-22 CPU-ms (tools/pipe_trace.py, round 2).  Planner on the device too: a
    // worker spends a third of a millisecond on a list and then sleeps until its PCM is down; 0.70-0.77 ms per list with 6,
    // 8, 12, 16 or 24 of them (round 3: the link is what bounds it).  Round 5 (tools/thread_cpu.py, three interleaved rounds of 1 500
    // lists): TWO of them 0.59-0.63 ms per list at 0.43-0.55 CPU-ms, three 0.65 / 0.67, eight 0.63-0.66 / 0.74-0.87 -- every worker has a
    // HIP stream of its own, the runtime spreads a process's streams over GPU_MAX_HW_QUEUES hardware queues per device, and once
    // streams share queues a thread of the RUNTIME orders them on the host: two pipelines with twelve streams each on one device (two
    // contexts of a node, or two ranks, sharing a card) kept that thread 65 % busy, 0.45 CPU-ms per list; with two stage-B workers a
    // pipeline has six streams.  (The context's own pipeline, which serves one waiting caller's parts side by side, keeps eight.)
    int nWorkers = (flags & DCS_PIPE_PLAN_ON_DEVICE)  ? std::min(depth, (flags & kPipeLatency) ? 8 : 2)
                 : (flags & DCS_PIPE_PACK_ON_DEVICE)  ? std::min(depth, std::max(4, dcs_host_threads() / 3))
                 : (flags & DCS_PIPE_INDEX_ON_DEVICE) ? std::min(depth, dcs_host_threads() + 4) : depth;
    // FLAC out, planner on the device: stage B holds a worker longer (the writer's kernels and, with the MD5, W4's serial walk run
    // behind the decode before anything comes down), so four of them: realistic_65536 at depth 32, two / three / four workers 0.81 /
    // 0.76 / 0.75 ms per list, with the MD5 1.66 / 1.32 / 1.16 (tools/flac_write_bench.py --pipeline).
    if ((flags & DCS_PIPE_FLAC) != 0 && (flags & DCS_PIPE_PLAN_ON_DEVICE) != 0 && (flags & kPipeLatency) == 0)
        nWorkers = std::min(depth, 4);
    if (pipeSwitches().workers != 0)
        nWorkers = pipeSwitches().workers;
    int nUploaders = 0;
    if (flags & DCS_PIPE_INDEX_ON_DEVICE)
    {
        // stage A costs a worker a quarter to half a millisecond per list: two of them keep up with any rate the link allows
        nUploaders = (flags & kPipeLatency) ? std::min(depth, 4) : depth >= 4 ? 2 : 1;      // (one waiting caller: its parts go up side by side)
        if (pipeSwitches().uploaders != 0)
            nUploaders = pipeSwitches().uploaders;
        nWorkers += nUploaders;
    }
    p->nUploaders = nUploaders;
    int prioLeast = 0, prioGreatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prioLeast, &prioGreatest);
    p->nWorkers = nWorkers;
    // two indexers, so that one round's walk runs while the other round's lists gather and its records come back
    const int nIndexers = (flags & DCS_PIPE_INDEX_ON_DEVICE) ? 2 : 0;
    for (int i = 0 ; i < nWorkers + nIndexers ; ++i)
    {
        hipStream_t s = nullptr;
        // The indexers' streams get the lowest and the highest priority: not for the priority, but because streams of
        // different priorities never share a hardware queue.  Their launches run for milliseconds (a walk is serial per
        // stream, on a handful of lanes), and neither a worker's copies and 40-microsecond kernels nor the other
        // indexer's launch must queue up behind one.
        // (DCS_PIPE_INDEXER_PRIO=ab, a / b one of l(east) g(reatest) n(ormal): the two indexers' priorities, an experiment switch)
        auto prioOf = [&](char c, int dflt) { return c == 'l' ? prioLeast : c == 'g' ? prioGreatest : c == 'n' ? (prioLeast + prioGreatest) / 2 : dflt; };
        const int idxPrio = i == nWorkers ? prioOf(pipeSwitches().indexerPrio[0], prioLeast) : prioOf(pipeSwitches().indexerPrio[1], prioGreatest);
        const hipError_t e = i >= nWorkers ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, idxPrio)
                                           : hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        if (e != hipSuccess)
        {
            for (hipStream_t t : p->streams) (void)hipStreamDestroy(t);
            delete p;
            setError(ctx, "dcs_pipeline_create: hipStreamCreate failed");
            return DCS_ERR_HIP;
        }
        p->streams.push_back(s);
    }
    for (int i = 0 ; i < nWorkers ; ++i)
        p->workers.emplace_back(pipelineWorker, p, i);
    for (int i = 0 ; i < nIndexers ; ++i)
        p->indexers.emplace_back(pipelineIndexer, p, i);
    *out = p;
    return DCS_OK;
}

extern "C" void dcs_pipeline_destroy(DcsPipeline *p)
{
    printWaitStats("dcs_pipeline_destroy");
    if (p == nullptr)
        return;
    {
        std::unique_lock<std::mutex> lk(p->m);
        // lists still in flight are finished first (their streams belong to the caller)
        p->finished.wait(lk, [&] { for (const DcsPipeline::JobPtr &j : p->order) if (!j->done) return false; return true; });
        p->quit = true;
    }
    p->work.notify_all();
    p->indexWork.notify_all();
    for (std::thread &w : p->workers)
        w.join();
    for (std::thread &t : p->indexers)
        t.join();
    (void)hipSetDevice(p->ctx->device);
    pipelineRelease(p->held);
    for (DcsPipeline::JobPtr &j : p->order)
        pipelineRelease(j);
    for (hipStream_t s : p->streams)
        (void)hipStreamDestroy(s);
    delete p;
}

static DcsStatus pipelineSubmit(DcsPipeline *p, const DcsStreamRef *streams, uint32_t nStreams, uint32_t extraFrames,
                                int16_t *pcmDst, uint32_t *errDst, const DcsFrameIndex *preRecords = nullptr,
                                const uint64_t *preFirstRecord = nullptr, const DcsStreamInfo *preInfos = nullptr)
{
    if (p == nullptr || streams == nullptr || nStreams == 0)
        return DCS_ERR_INVALID_ARG;
    DcsPipeline::JobPtr job = std::make_shared<DcsPipeline::Job>();
    job->streams = streams; job->nStreams = nStreams; job->extraFrames = extraFrames;
    job->pcmDst = pcmDst; job->errDst = errDst;
    job->preRecords = preRecords; job->preFirstRecord = preFirstRecord; job->preInfos = preInfos;
    const double ts0 = nowMs();
    {
        std::unique_lock<std::mutex> lk(p->m);
        // at most `depth` lists between submit and collect (each holds device and pinned buffers)
        p->room.wait(lk, [&] { return static_cast<int>(p->order.size()) < p->depth; });
        job->tSubmit = nowMs();
        pipeLog("caller", 0, "submit-wait", ts0, job->tSubmit);
        p->fresh.push_back(job);
        p->order.push_back(job);
    }
    p->work.notify_all();           // (workers have roles: the one woken must be one that takes fresh lists)
    return DCS_OK;
}

extern "C" DcsStatus dcs_pipeline_submit(DcsPipeline *p, const DcsStreamRef *streams, uint32_t nStreams, uint32_t extraFrames)
{
    return pipelineSubmit(p, streams, nStreams, extraFrames, nullptr, nullptr);
}

// the oldest list, once it is finished, becomes the one the caller reads (the previous one's buffers go back to the context's cache)
static DcsStatus pipelineTakeOldest(DcsPipeline *p, DcsPipeline::JobPtr &job)
{
    const double tc0 = nowMs();
    (void)hipSetDevice(p->ctx->device);
    const double tc1 = nowMs();
    pipelineRelease(p->held);
    pipeLog("caller", 0, "set-device", tc0, tc1);
    pipeLog("caller", 0, "release", tc1, nowMs());
    {
        std::unique_lock<std::mutex> lk(p->m);
        if (p->order.empty())
            return DCS_ERR_INVALID_ARG;             // nothing submitted
        job = p->order.front();
        p->finished.wait(lk, [&] { return job->done; });
        p->order.pop_front();
    }
    p->room.notify_one();
    p->held = job;
    return DCS_OK;
}

// collect: the oldest list becomes the held one, and what both kinds of result have in common is filled in
template <class Result>
static DcsStatus pipelineCollect(DcsPipeline *p, Result *out, DcsPipeline::JobPtr &job)
{
    const DcsStatus taken = pipelineTakeOldest(p, job);
    if (taken != DCS_OK)
        return taken;
    memset(out, 0, sizeof(*out));
    out->status = job->status;
    out->nStreams = job->nStreams;
    out->hostMs = static_cast<float>(job->hostMs);
    out->path = job->path;
    out->deviceMs = static_cast<float>(job->deviceMs);
    if (job->status == DCS_OK)
    {
        out->err = job->err;
        out->frameOffsets = job->firstJob.data();
        out->nFrames = job->firstJob.empty() ? 0u : job->firstJob.back();
    }
    return job->status;
}

extern "C" DcsStatus dcs_pipeline_collect(DcsPipeline *p, DcsPipelineResult *out)
{
    if (p == nullptr || out == nullptr || (p->flags & DCS_PIPE_FLAC) != 0)     // (a FLAC pipeline's lists are dcs_pipeline_collect_flac's)
        return DCS_ERR_INVALID_ARG;
    DcsPipeline::JobPtr job;
    const DcsStatus st = pipelineCollect(p, out, job);
    if (job && st == DCS_OK)
        out->pcm = job->pcm;
    return st;
}

extern "C" DcsStatus dcs_pipeline_collect_flac(DcsPipeline *p, DcsPipelineFlacResult *out)
{
    if (p == nullptr || out == nullptr || (p->flags & DCS_PIPE_FLAC) == 0)
        return DCS_ERR_INVALID_ARG;
    DcsPipeline::JobPtr job;
    const DcsStatus st = pipelineCollect(p, out, job);
    if (job && st == DCS_OK)
    {
        out->flac = job->flac.bytes();
        out->flacOffsets = job->flac.offsets();
        out->info = job->flac.info();
    }
    return st;
}

// dcs_decode_streams for a LARGE list, in parts through the context's own pipeline
#include "dcs_large_list.hip.h"
