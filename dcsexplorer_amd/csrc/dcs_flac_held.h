// dcs_flac_held.h -- FlacHeld, the owner of everything one queued run of the FLAC writer (dcs_flac_write.hip.h) borrows from a
// context's buffer cache, and dcsFlacWriteQueue, the one statement of what such a run queues.  Shared by dcs_encode.hip's unit
// (the writer) and dcs_runtime.hip's (the pipeline, whose lists keep theirs until they are collected, as Job::hBlob).
#pragma once
#include <stdint.h>
#include "../../include/dcs_hip.h"
#include "dcs_cache.h"

// Nothing here waits: whoever lets it go while work queued on the run's stream may still use it waits for that stream first.
// After that wait the pinned side holds the result: the table as the ABI lays it out (outOffsets, nStreams + 1; the total
// in a word of its own; DcsFlacWriteInfo, nStreams) and the FLAC bytes, total() of them.
struct FlacHeld
{
    CacheBuf dWork;                         // offsets and block table as uploaded, W1's records, W2's places and sums, bases, digests, the table
    CacheBuf dOut;                          // the FLAC bytes in HBM, sized by the bound
    CacheBuf hUp, hTable, hOut;             // pinned: what goes up, the table and the FLAC bytes as they come down
    uint32_t n = 0;
    uint64_t bound = 0;                     // what the streams can come to at most (the host knows it before anything runs)

    const uint64_t *offsets() const { return hTable.as<const uint64_t>(); }
    uint64_t total() const { return offsets()[static_cast<size_t>(n) + 1]; }
    const DcsFlacWriteInfo *info() const { return reinterpret_cast<const DcsFlacWriteInfo *>(offsets() + static_cast<size_t>(n) + 2); }
    const uint8_t *bytes() const { return hOut.as<const uint8_t>(); }
    static size_t tableBytes(uint32_t n) { return sizeof(uint64_t) * (static_cast<size_t>(n) + 2) + sizeof(DcsFlacWriteInfo) * n; }
    explicit operator bool() const { return static_cast<bool>(hTable); }
    void release()
    {
        for (CacheBuf *c : { &dWork, &dOut, &hUp, &hTable, &hOut })       // (in this order: the cache evicts what came back first)
            c->release();
        n = 0;
        bound = 0;
    }
};

// Among dcsFlacWriteQueue's and dcsFlacWriteFromDevice's flags, beside DCS_FLAC_MD5, and no flag of the ABI: the streams are
// of any length from 1 sample on (a converter's output), not whole frames of 240.
constexpr uint32_t kFlacWriteAnyLength = 0x80000000u;

// Queues, on `stream` and behind whatever produces dPcm there, the whole writer for stream k = dPcm[sampleOffsets[k] ..
// sampleOffsets[k + 1]) (offsets on the host, copied before this returns): the upload of offsets and block table, W1, W2, the
// scan across streams, W4 with DCS_FLAC_MD5, the stream heads, W3, and the table's and the FLAC bytes' way down into `held`'s
// pinned memory (the latter by at most downBlocks workgroups).  Returns without waiting; nStreams >= 1.  On failure something
// may have been queued all the same: wait for the stream before `held` goes.
DcsStatus dcsFlacWriteQueue(DcsCtx *ctx, hipStream_t stream, const int16_t *dPcm, const uint64_t *sampleOffsets, uint32_t nStreams,
                            uint32_t rate, uint32_t flags, FlacHeld &held, unsigned downBlocks);

// ... and its sampleOffsets for decoded streams: from the first output frame of every stream and their total (nStreams + 1 entries)
inline void dcsFlacSampleOffsets(const uint32_t *firstJob, uint32_t nStreams, std::vector<uint64_t> &sampleOffsets)
{
    sampleOffsets.resize(static_cast<size_t>(nStreams) + 1);
    for (uint32_t k = 0 ; k <= nStreams ; ++k)
        sampleOffsets[k] = static_cast<uint64_t>(firstJob[k]) * DCS_FRAME_SAMPLES;
}
