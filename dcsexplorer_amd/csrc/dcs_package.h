// dcs_package.h -- the chunk plan and the chunk package: what a decode launch is handed, stated once for the host planner and
// packer (dcs_plan.cpp) and for the device planner and packer (dcs_plan_device.hip.h).  Plain C++17; the rules are force-inlined
// functions that compile for both sides.  The drivers decide how the work is spread (threads, lanes, 16-byte moves); what a slot,
// a run, a split record or an image dword IS is decided here.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/dcs_hip.h"

#ifdef __cplusplus
#ifdef __HIPCC__
#define DCS_HD __host__ __device__
#else
#define DCS_HD
#endif
#define DCS_HDI static inline __attribute__((always_inline)) DCS_HD
// an index record seen as dwords (its fields are read in pairs and fours)
typedef uint32_t __attribute__((may_alias)) DcsRecDword;
#endif

// ---------------------------------------------------------------------------------------------
// Kernel work list.  The planner (dcs_plan.cpp) cuts the job list into chunks of at most FPW slots;
// one wavefront decodes one chunk.  A slot is a job to decode; HALO slots are decoded only for the
// 16-sample tail they hand to a later slot of the same chunk (the predecessor of the chunk's first
// frame lives in another chunk).
// ---------------------------------------------------------------------------------------------
// LDS bit pool: the compressed bytes of the frames one wavefront unpacks in one round are staged
// there.  The planner closes a chunk before the pool would overflow.
#define DCS_POOL_DW_PER_FRAME 56        // 224 bytes per frame slot on average (typical frame: ~125-150 bytes)
#define DCS_POOL_DW_MIN       320       // but never less than two maximal frames (a halo and its successor)
#define DCS_MAX_FRAME_BITS    4480      // 16 band headers + 255 x 16-bit samples, rounded up

#define DCS_SLOT_HALO      0x01u        // do not write PCM / err for this slot
#define DCS_SLOT_EXT_TAIL  0x02u        // overlap tail comes from tailsIn[job.prev & 0x7FFFFFFF]
#define DCS_SLOT_EXPORT    0x04u        // this frame's tail meets a frame of another chunk (job nextJob) at handoff[this chunk]
#define DCS_SLOT_IMPORT    0x08u        // overlap tail meets this frame at handoff[prevJob] (prevJob = the chunk of its predecessor)
#define DCS_SLOT_KEEP_TAIL 0x10u        // store this frame's tail in tailsOut: the last frame of its chain in the batch (what a caller
                                        // needs to carry a stream into its next batch), or every frame when the batch keeps all tails
#define DCS_SLOT_EMPTY     0x80u        // padding
#define DCS_NO_PREV_SLOT   0xFFu

struct DcsSlot                          // 32 bytes: everything the kernel needs to know about a job, so
{                                       // that the job list itself is never read on the device
    uint32_t job;                       // output index (PCM row, err entry)
    uint8_t  prevSlot;                  // slot index inside the chunk whose tail overlaps into this one
    uint8_t  flags;
    uint8_t  nSrc;
    uint8_t  shiftXform;                // volShift | xform << 4
    uint32_t firstSrc;
    uint32_t prevJob;                   // DcsFrameJob.prev (external-tail index when DCS_SLOT_EXT_TAIL)
    // Unpack round 0 (the FIRST source of every job), worked out by the planner so that nothing of it waits for
    // the descriptor.  The compressed bytes of a chunk's frames mostly lie back to back in the blob (consecutive
    // frames of one stream), so they are staged as RUNS of dwords, 16 bytes per lane: slot k of a chunk carries
    // run k (runNDw == 0: no further run), which has nothing to do with slot k's own frame.
    uint32_t runStartDw;                // first blob dword of run k
    uint16_t runNDw;                    // its length in dwords (whole frames + 3 dwords of window look-ahead)
    uint16_t poolOff;                   // THIS slot's frame: pool dword that holds its first bit
    uint32_t nextJob;                   // DCS_SLOT_EXPORT: the job whose first 16 samples this frame's tail overlaps into (round 6; the
                                        // field held the blob dword of the stream header, which both packers take from the source)
    uint8_t  pad_;
    uint8_t  bpl;                       // header bands per unpack lane (dcsBandsPerLane); 0: one lane unpacks the whole frame
    uint16_t runPoolOff;                // pool dword where run k goes (a multiple of 4)
};

// A source as the planner and the DEVICE packer need it when the index records stay on the device (the pipeline's
// device path): 24 bytes instead of the 160 of DcsSrcDesc.  `record` = index of the frame's DcsFrameIndex in the
// device-resident record array.
struct DcsPlanSrc
{
    uint64_t streamOff;
    uint32_t bitOff;
    uint16_t nBits;
    uint8_t  hdrLen, nBands, flags, format;
    uint16_t mixMul;
    uint32_t record;
};
// What the arithmetic planner (dcsPlanChunk below; dcsPlanKernel, dcs_plan_device.hip.h) is told about a stream of a list of
// whole streams -- everything the host knows without walking the stream: where it lies, its frame count, layout and mixing
// parameters.  40 bytes.
struct DcsPlanStream
{
    uint64_t streamOff;                 // offset of the stream in the list's blob
    uint32_t len;                       // bytes that belong to it
    uint32_t firstRecord;               // its records in the list's record array
    uint32_t firstJob;                  // its first output frame
    uint32_t nFrames;                   // the stream's U16 frame count (output frames: nFrames + extraFrames)
    uint16_t mixMul0, mixMulN;          // rescaled mixing multiplier of frame 0 / of every later frame (dcs_stream_params_from)
    uint8_t  volShift0, volShiftN;
    uint8_t  xform, hdrLen, format, pad_[3];
};
static_assert(sizeof(DcsPlanStream) == 40, "DcsPlanStream layout (uploaded by copy kernel: whole dwords)");
#define DCS_PLAN_POOL_OVERFLOW 1u       // flag word of the arithmetic planner: some chunk's compressed bytes do not fit the bit pool
#define DCS_PLAN_TRUNCATED     2u       // ... some stream's frames run past its buffer

#ifdef __cplusplus
// dwords of pool one source occupies: whole dwords covering the frame + 3 dwords of window look-ahead
DCS_HDI uint32_t dcsPoolDwords(uint64_t streamOff, uint32_t hdrLen, uint32_t bitOff, uint32_t nBits)
{
    const uint32_t inDword = static_cast<uint32_t>(((streamOff + 2 + hdrLen) * 8 + bitOff) & 31);
    return (inDword + nBits + 31) / 32 + 3;
}
// ... and the blob dword that holds the frame's first bit
DCS_HDI uint32_t dcsFrameFirstDword(uint64_t streamOff, uint32_t hdrLen, uint32_t bitOff)
{
    return static_cast<uint32_t>(((streamOff + 2 + hdrLen) * 8 + bitOff) >> 5);
}
DCS_HDI constexpr uint32_t dcsPoolCapacity(int fpw)
{
    return static_cast<uint32_t>(fpw * DCS_POOL_DW_PER_FRAME > DCS_POOL_DW_MIN ? fpw * DCS_POOL_DW_PER_FRAME : DCS_POOL_DW_MIN);
}

// Header bands per unpack lane of a frame, ceil(min(nBands, 16) / (64 / fpw)); 0: one lane unpacks the whole frame (DCS_IDX_SERIAL)
DCS_HDI constexpr uint8_t dcsBandsPerLane(uint32_t nBands, uint32_t idxFlags, int fpw)
{
    const uint32_t sub = 64u / static_cast<uint32_t>(fpw), nb16 = nBands < 16 ? nBands : 16, bpl = (nb16 + sub - 1) / sub;
    return (idxFlags & DCS_IDX_SERIAL) ? 0 : static_cast<uint8_t>(bpl < 1 ? 1 : bpl);
}

// Run placement.  Unpack round 0 is staged as runs of blob dwords: a frame that starts inside or right behind the chunk's last
// run extends it, anything else opens a new run at the next 16-byte boundary of the pool.  There are never more runs than frames
// placed, so run k rides in slot k of the chunk: store() it there whenever place() has opened or grown it.
struct DcsRunCursor
{
    uint32_t start = 0, n = 0, off = 0; // the chunk's last run: first blob dword, dwords, pool dword where it goes
    uint32_t nRuns = 0;
    uint32_t use = 0;                   // pool dwords the runs take

    DCS_HD bool extends(uint32_t firstDw) const { return nRuns != 0 && firstDw >= start && firstDw <= start + n; }
    // the frame's poolOff
    DCS_HD uint32_t place(uint32_t firstDw, uint32_t nDw)
    {
        if (extends(firstDw))
            n = firstDw + nDw > start + n ? firstDw + nDw - start : n;
        else
        {
            start = firstDw; n = nDw; off = use;
            ++nRuns;
        }
        use = off + ((n + 3) & ~3u);
        return off + (firstDw - start);
    }
    // the pool use place() would leave; `from` other than `use`: the use with a frame in front that has not been placed (a halo
    // in front of its successor), behind which this frame counts as a run of its own
    DCS_HD uint32_t useWith(uint32_t firstDw, uint32_t nDw, uint32_t from) const
    {
        if (from != use || !extends(firstDw))
            return from + ((nDw + 3) & ~3u);
        const uint32_t len = firstDw + nDw > start + n ? firstDw + nDw - start : n;
        return off + ((len + 3) & ~3u);
    }
    DCS_HD void store(DcsSlot &sl) const
    {
        sl.runStartDw = start;
        sl.runNDw = static_cast<uint16_t>(n);
        sl.runPoolOff = static_cast<uint16_t>(off);
    }
};

// Which header bands the q-th unpack lane of a frame takes: lane q starts at dcsLaneFirstBand(q) and ends where lane
// q + 1 starts.  The 1993 layouts (sixteen bands of sixteen samples) get bpl consecutive bands per lane.  The bands of a
// 1994+ frame hold 7, 8, 13 x 16 and 32 samples: there bands 0 and 1 count as one and band 15 as two, which with eight
// lanes gives {0, 1, 2} {3, 4} ... {13, 14} {15}, 31 or 32 samples for every lane (the symbol loop works through them in
// rounds of 7, 9 and 16 samples, unpack94 in dcs_kernels.hip.h).  With sixteen lanes it is {0, 1} {2} ... {14} {15} and
// the last lane is left for the second half of band 15, which the packers give it when the index pass recorded where
// that half starts (dcsMid15: split[14].prv / .prvDelta, dcs_scan.h).
DCS_HDI constexpr int dcsLaneFirstBand(int format, int q, int bpl, int nbEnd)
{
    // OS93a Type 1: eighteen bands of 2, 2, 2, 2, 3, 4, 5, 6, 5, 6, 7, 9, 11, 14, 12, 12, 12, 13 sample pairs
    // (DCSDecoderNative.cpp:2865).  The lanes of a wavefront walk their k-th bands together, so what counts is the
    // longest k-th band: {0,1,2} {3,4,5} {6,7} {8,9} ... {16,17} with eight lanes (12 + 14 + 4 pairs; two bands per
    // lane in order cost 12 + 14 + 12 + 13), {0,1} {2,3} {4} {5} ... {17} with sixteen, {0..6} {7..10} {11..13} {14..17}
    // with four.  (nbEnd: 18 or the stream's own band count.)
    if (format == DCS_FMT_93A_T1)
    {
        const int b = bpl == 1 ? (q < 2 ? 2 * q : q + 2) : bpl == 2 ? (q < 2 ? 3 * q : 2 * q + 2) : (q == 0 ? 0 : q == 1 ? 7 : q == 2 ? 11 : 14);
        return b < nbEnd ? b : nbEnd;
    }
    const int b = q * bpl + ((format >= DCS_FMT_94_T0 && q != 0) ? 1 : 0);
    return b < nbEnd ? b : nbEnd;
}
// the band where the lanes' dealing ends: sixteen header bands, eighteen for OS93a Type 1
DCS_HDI constexpr int dcsDealEnd(int format, int nBands)
{
    return format == DCS_FMT_93A_T1 ? (nBands < 18 ? nBands : 18) : (nBands < 16 ? nBands : 16);
}
// OS93a Type 1: a lane's first band can be 16 or 17; then this bit of its state word is set and bits 12..15 hold band - 16
// (the record itself comes from the frame record's bandType bytes, dcs_scan.h)
#define DCS_SPLIT_BASE16 0x200u
// state word of a lane that starts in the middle of band 15: output index | DCS_MID15_STRADDLE (bit 9) | this flag
#define DCS_SPLIT_MID15 0x800u
#define DCS_MID15_STRADDLE 0x200u
// ... and whether the frame's last lane does: one band per lane, all sixteen bands, a recorded middle
DCS_HDI constexpr bool dcsMid15(int format, int bpl, int nb16, uint32_t midBits)
{
    return format >= DCS_FMT_94_T0 && bpl == 1 && nb16 == 16 && midBits != 0;
}

// The EVEN deal of a 1994+ frame to eight lanes (first source, 8 frames per wavefront, a batch with DCS_BATCH_EVEN_DEAL).
// Whole bands cannot be dealt more evenly than 31 or 32 samples for the fullest lane, however few of the sixteen bands the
// stream codes; UNITS of 8 samples can: band 0 (7 samples), band 1, and the two halves of every later band (a strided band's
// halved count still makes two halves).  A frame of nb header bands has dcsEvenUnits(nb) of them; lane q takes
// dcsLaneUnits(nb, q).count consecutive ones from .first on: ceil(units / 8) or one fewer, in order.  A lane that starts with
// a second half needs the decoder's state in the middle of that band: the mid records (DcsFrameMids, which the host index
// walk records as it passes each middle: dcsScan94<MIDS>, through dcs_index_stream_mids).  The symbol loop then runs in rounds of 8 samples.
// Today's deal stays for a frame with all sixteen bands (band 15's halves are 16 samples: units do no better than 32 there),
// for one without mid records or in error, for the 1993 layouts and for the further sources of a frame.
struct DcsUnitRange { int first, count; };
DCS_HDI constexpr int dcsEvenUnits(int nb) { return nb < 2 ? nb : 2 * nb - 2; }
DCS_HDI constexpr DcsUnitRange dcsLaneUnits(int nb, int q)
{
    const int units = dcsEvenUnits(nb), lo = units >> 3, extra = units & 7;
    return DcsUnitRange{ q * lo + (q < extra ? q : extra), lo + (q < extra ? 1 : 0) };
}
DCS_HDI constexpr int dcsUnitBand(int u) { return u < 2 ? u : 1 + (u >> 1); }
DCS_HDI constexpr int dcsUnitHalf(int u) { return u < 2 ? 0 : (u & 1); }
// mid[0] of a frame's DcsFrameMids: set when the walk recorded the middle of every band it has
#define DCS_MIDS_VALID 1u
DCS_HDI constexpr bool dcsEvenDealt(int format, int bpl, int nb16, int sub, const uint32_t *mid)
{
    return format >= DCS_FMT_94_T0 && bpl != 0 && sub == 8 && nb16 < 16 && mid != nullptr && mid[0] == DCS_MIDS_VALID;
}

// Where a 1994+ frame's bands lie in its tile row: band 0 (7 samples) from word 1 on, band 1 (8) from word 8, bands 2..14 (16
// each) from word 16 (b - 1), band 15 (32) up to word 255.  dcsBandFirstWord: a band's first word; dcsLastWord: the last word
// a frame of nb header bands can fill.
DCS_HDI constexpr int dcsBandFirstWord(int b) { return b <= 0 ? 1 : b == 1 ? 8 : 16 * (b - 1); }
DCS_HDI constexpr int dcsLastWord(int nb) { return nb <= 0 ? 0 : nb == 1 ? 7 : nb >= 16 ? 255 : 15 + 16 * (nb - 2); }
// The pre-pass of the 1994+ transform pairs point i = l + 8 j (lane l = 0..7 of the frame, j = 0..7) with point 128 - i, a point
// being a dword of the row.  Where no row holds more than nb bands, the partners of the first dcsPrepassShort(nb) values of j
// are zero in every lane: the lowest of them, 128 - (7 + 8 j), lies behind the last word filled.
DCS_HDI constexpr int dcsPrepassShort(int nb)
{
    const int firstFree = (dcsLastWord(nb) + 2) / 2;        // the first point without a filled word
    int zj = 0;
    while (zj < 8 && 128 - (7 + 8 * zj) >= firstFree)
        ++zj;
    return zj;
}
// the most bands for which at least `zj` values of j are short (0: none)
DCS_HDI constexpr int dcsPrepassBands(int zj)
{
    int nb = 16;
    while (nb > 0 && dcsPrepassShort(nb) < zj)
        --nb;
    return nb;
}

// Chunk packages.  Everything unpack round 0 of a chunk needs, gathered once per batch by the host packer
// (dcsBuildPackages, dcs_plan.cpp) or the device packer (dcsPackKernel) into one block at a fixed stride, so that a wavefront
// requests ALL of it at its first instruction (no load depends on another load).  Round 5 layout (a wavefront reads its whole
// package, so every byte of it counts as HBM traffic):
//   [0, fpw x 80)   per slot five 16-byte pieces: the slot (DcsSlot bytes 0..15: job, prevSlot | flags | nSrc | shiftXform,
//                   firstSrc, prevJob) | descriptor head bytes 0..15 | 16..31 | 32..39 followed by poolOff (u16), bpl (u8),
//                   a spare byte and nextJob (u32) | the stream header (16 B, a 1-byte header zero-extended)
//   [fpw x 80, ..)  the split record of every lane [64]: 8 bytes (zero for a frame's first lane; the lane's first band in bits
//                   12..15 of its state word, bit 15 of bitDelta: no bands) -- or, when every source of the batch is a 1994+
//                   frame, 4 bytes: bitDelta | state << 16 (those layouts carry nothing in prv / prvDelta but band 15's middle,
//                   which the packers fold into the two halves)
//   [dcsPkgOffPool, + imgDw x 4)  the image of the bit pool (runs placed, dwords in bit order), as long as the batch's fullest
//                   chunk needs, a multiple of 128 bytes (a HOST-planned batch; one planned on the device has the pool's capacity:
//                   its stride would have to come out of device memory, a dependent load in front of the package loads)
// The layout word: image dwords | DCS_PKG_SPLIT4; it travels to the kernel in bits 16..31 of its flags.
#define DCS_PKG_SLOT_BYTES 80u
#define DCS_PKG_SLOT_DWORDS 20
#define DCS_PKG_SPLIT4     0x8000u
DCS_HDI constexpr uint32_t dcsPkgImgDw(uint32_t layout) { return layout & 0x7FFFu; }
DCS_HDI constexpr uint32_t dcsPkgSplitBytes(uint32_t layout) { return (layout & DCS_PKG_SPLIT4) ? 4u : 8u; }
DCS_HDI constexpr uint32_t dcsPkgOffSplit(int fpw) { return static_cast<uint32_t>(fpw) * DCS_PKG_SLOT_BYTES; }
DCS_HDI constexpr uint32_t dcsPkgOffPool(int fpw, uint32_t layout)
{
    return (static_cast<uint32_t>(fpw) * DCS_PKG_SLOT_BYTES + 64u * dcsPkgSplitBytes(layout) + 127u) & ~127u;
}
DCS_HDI constexpr uint32_t dcsPkgStride(int fpw, uint32_t layout) { return dcsPkgOffPool(fpw, layout) + dcsPkgImgDw(layout) * 4u; }

// The first source of a slot's job as a package sees it, from either form of source record: the descriptor of the ABI, or the
// digest beside the device-resident records.  rec == nullptr: the slot has none.
struct DcsPkgSrc
{
    uint64_t streamOff;
    uint32_t mixMul, format, hdrLen, nBands;
    const DcsFrameIndex *rec;
    const uint32_t *mid;                // the frame's DcsFrameMids, or null: whole bands only (dcsEvenDealt)
};
DCS_HDI bool dcsSlotHasSrc(const DcsSlot &sl) { return !(sl.flags & DCS_SLOT_EMPTY) && sl.nSrc != 0; }
DCS_HDI DcsPkgSrc dcsPkgSrcOf(const DcsSlot &sl, const DcsSrcDesc *srcs, const DcsFrameMids *mids = nullptr)
{
    if (!dcsSlotHasSrc(sl) || srcs == nullptr)
        return DcsPkgSrc{ 0, 0, 0, 0, 0, nullptr, nullptr };
    const DcsSrcDesc &sd = srcs[sl.firstSrc];
    return DcsPkgSrc{ sd.streamOff, sd.mixMul, sd.format, sd.hdrLen, sd.idx.nBands, &sd.idx,
                      mids != nullptr ? mids[sl.firstSrc].mid : nullptr };
}
DCS_HDI DcsPkgSrc dcsPkgSrcOf(const DcsSlot &sl, const DcsPlanSrc *srcs, const DcsFrameIndex *records)
{
    if (!dcsSlotHasSrc(sl))
        return DcsPkgSrc{ 0, 0, 0, 0, 0, nullptr, nullptr };
    const DcsPlanSrc sd = srcs[sl.firstSrc];
    return DcsPkgSrc{ sd.streamOff, sd.mixMul, sd.format, sd.hdrLen, sd.nBands, &records[sd.record], nullptr };
}

// The 80-byte slot entry as dwords (five 16-byte pieces): slot bytes 0..15 | the 40-byte descriptor head -- what DcsSrcDesc
// holds in front of the split records: streamOff, mixMul | format << 16 | hdrLen << 24, then the record's bitOff, nBits |
// hdrBits, bandType[16], preAdj | nBands | flags -- | poolOff | bpl << 16 | nextJob | the stream header.  Zero where the slot
// has no source; header bytes at or past blobLen read as zero.
#define DCS_PKG_HEAD_DWORDS 10
static_assert(offsetof(DcsSlot, runStartDw) == 16 && sizeof(DcsSlot) == 32, "the entry's first piece is the slot's first half");
static_assert(offsetof(DcsSrcDesc, mixMul) == 8 && offsetof(DcsSrcDesc, format) == 10 && offsetof(DcsSrcDesc, hdrLen) == 11
              && offsetof(DcsSrcDesc, idx) == 12, "descriptor head: three dwords in front of the record");
static_assert(offsetof(DcsSrcDesc, idx) + offsetof(DcsFrameIndex, split) == 4 * DCS_PKG_HEAD_DWORDS && offsetof(DcsFrameIndex, bandType) == 8,
              "descriptor head: the record up to its split records");
static_assert(16 + 4 * DCS_PKG_HEAD_DWORDS + 8 + 16 == DCS_PKG_SLOT_BYTES && DCS_PKG_SLOT_DWORDS * 4 == DCS_PKG_SLOT_BYTES, "slot entry");
DCS_HDI void dcsPkgSlotEntry(uint32_t e[DCS_PKG_SLOT_DWORDS], const DcsSlot &sl, const DcsPkgSrc &sd, const uint8_t *blob, uint64_t blobLen)
{
    __builtin_memcpy(e, &sl, 16);                   // job, prevSlot | flags | nSrc | shiftXform, firstSrc, prevJob
#pragma unroll
    for (int i = 4 ; i < DCS_PKG_SLOT_DWORDS ; ++i)
        e[i] = 0;
    e[14] = static_cast<uint32_t>(sl.poolOff) | (static_cast<uint32_t>(sl.bpl) << 16);
    e[15] = sl.nextJob;
    if (sd.rec == nullptr)
        return;
    e[4] = static_cast<uint32_t>(sd.streamOff);
    e[5] = static_cast<uint32_t>(sd.streamOff >> 32);
    e[6] = sd.mixMul | (sd.format << 16) | (sd.hdrLen << 24);
    const DcsRecDword *rec = reinterpret_cast<const DcsRecDword *>(sd.rec);
#pragma unroll
    for (int i = 0 ; i < DCS_PKG_HEAD_DWORDS - 3 ; ++i)
        e[7 + i] = rec[i];
    const uint64_t hOff = sd.streamOff + 2;
    const uint32_t hLen = sd.hdrLen == 1 ? 1u : 16u;
#pragma unroll
    for (uint32_t i = 0 ; i < 16 ; ++i)
        if (i < hLen && hOff + i < blobLen)
            e[16 + (i >> 2)] |= static_cast<uint32_t>(blob[hOff + i]) << (8 * (i & 3));
}

// The split record (r[0] = bitDelta | prv << 16, r[1] = prvDelta | state << 16) of a frame's q-th unpack lane of `sub`: where
// its first band (dcsLaneFirstBand) starts, that band in bits 12..15 of the state word.  Zero for the first lane, for a frame one
// lane unpacks alone (bpl == 0) and for a slot without a source; bit 15 of bitDelta: no bands for this lane.
DCS_HDI void dcsLaneSplit(uint32_t r[2], const DcsPkgSrc &sd, int bpl, int q, int sub)
{
    r[0] = r[1] = 0;
    if (sd.rec == nullptr || bpl == 0 || q < 1 || q >= sub)
        return;
    const int format = static_cast<int>(sd.format), nBands = static_cast<int>(sd.nBands);
    const int nbEnd = dcsDealEnd(format, nBands), base = dcsLaneFirstBand(format, q, bpl, nbEnd);
    const DcsRecDword *split = reinterpret_cast<const DcsRecDword *>(sd.rec->split), *mid = split + 2 * 14;
    if (dcsEvenDealt(format, bpl, nbEnd, sub, sd.mid))
    {
        // the even deal: the lane's first unit is a band, whose record is the band's, or the second half of one, whose
        // record is the mid record in the form of band 15's below
        const DcsUnitRange u = dcsLaneUnits(nbEnd, q);
        const int band = dcsUnitBand(u.first);
        if (u.count == 0)
            r[0] = 0x8000u;
        else if (dcsUnitHalf(u.first) != 0)
        {
            r[0] = sd.mid[band] & 0xFFFFu;
            r[1] = (((sd.mid[band] >> 16) & 0x3FFu) | DCS_SPLIT_MID15 | (static_cast<uint32_t>(band) << 12)) << 16;
        }
        else
        {
            const DcsRecDword *sp = split + 2 * (band - 1);
            r[0] = sp[0];
            r[1] = (sp[1] & 0x0FFFFFFFu) | (static_cast<uint32_t>(band) << 28);
        }
    }
    else if (q == sub - 1 && dcsMid15(format, bpl, nBands < 16 ? nBands : 16, mid[0] >> 16))
    {
        // the second half of band 15 (1994+, one band per lane): split[14].prv / .prvDelta
        r[0] = mid[0] >> 16;
        r[1] = ((mid[1] & 0x3FFu) | DCS_SPLIT_MID15 | (15u << 12)) << 16;
    }
    else if (base >= nbEnd)
        r[0] = 0x8000u;
    else if (base >= 16)
    {
        // OS93a Type 1, bands 16 and 17: their records travel in the frame record's bandType bytes
        const DcsRecDword *sp = reinterpret_cast<const DcsRecDword *>(sd.rec->bandType) + 2 * (base - 16);
        r[0] = sp[0];
        r[1] = (sp[1] & 0x0DFFFFFFu) | (DCS_SPLIT_BASE16 << 16) | (static_cast<uint32_t>(base - 16) << 28);
    }
    else
    {
        const DcsRecDword *sp = split + 2 * (base - 1);
        r[0] = sp[0];
        r[1] = (sp[1] & 0x0FFFFFFFu) | (static_cast<uint32_t>(base) << 28);
    }
}
// ... and its 4-byte form (DCS_PKG_SPLIT4): bitDelta | state << 16
DCS_HDI uint32_t dcsLaneSplit4(const uint32_t r[2]) { return (r[0] & 0xFFFFu) | (r[1] & 0xFFFF0000u); }

// Dword i of the blob as the pool image holds it: in bit order (big-endian), bytes at or past blobLen reading as zero.
// dcsImageDwordInside: the same for a dword that is known to lie inside the blob.
DCS_HDI uint32_t dcsImageDwordInside(const uint8_t *blob, uint64_t i)
{
    uint32_t w;
    __builtin_memcpy(&w, blob + i * 4, 4);
    return __builtin_bswap32(w);
}
DCS_HDI uint32_t dcsImageDword(const uint8_t *blob, uint64_t blobLen, uint64_t i)
{
    const uint64_t b0 = i * 4;
    if (b0 + 4 <= blobLen)
        return dcsImageDwordInside(blob, i);
    uint32_t w = 0;
    for (int j = 0 ; j < 4 ; ++j)
        if (b0 + j < blobLen)
            w |= static_cast<uint32_t>(blob[b0 + j]) << (24 - 8 * j);
    return w;
}

// The arithmetic plan of one chunk of a list of WHOLE STREAMS.  The job list of such a list is regular -- stream k's frames
// f = 0 .. nFrames + extraFrames - 1 one after the other, each the successor of the one before -- so chunk c holds jobs
// c * fpc .. c * fpc + fpc - 1 (fpc: frames a chunk holds, FPW or -- for a list whose frames are too large for FPW of them to
// share the bit pool -- fewer; the chunk's other slots stay empty), and a frame whose predecessor lies in the chunk before imports
// its tail from there.  Fills out[FPW] and the source digests of the chunk's frames (srcs[record]); returns DCS_PLAN_* flags for
// what the arithmetic plan cannot express, and the list then takes the chain planner's path (dcs_plan.cpp): a chunk whose
// compressed bytes overflow the bit pool (the chain planner closes such a chunk early), a stream whose frames run past its buffer.
// A stream the index pass stopped early (nValidFrames < nFrames) needs no flag: its remaining frames are silent here as there.
DCS_HDI constexpr uint32_t dcsMin(uint32_t a, uint32_t b) { return a < b ? a : b; }
template <int FPW>
DCS_HDI uint32_t dcsPlanChunk(const DcsPlanStream *streams, uint32_t nStreams, const DcsStreamInfo *infos, const DcsFrameIndex *records,
                              uint32_t extraFrames, uint32_t nJobs, uint32_t fpc, uint32_t c, DcsSlot out[FPW], DcsPlanSrc *srcs)
{
    // the stream of the chunk's first job: the last stream whose first job is not behind it
    uint32_t lo = 0, hi = nStreams - 1;
    const uint32_t j0 = c * fpc;
    while (lo < hi)
    {
        const uint32_t mid = (lo + hi + 1) / 2;
        if (streams[mid].firstJob <= j0) lo = mid; else hi = mid - 1;
    }
    uint32_t k = lo;
    DcsPlanStream st = streams[k];
    uint32_t nValid = dcsMin(static_cast<uint32_t>(infos[k].nValidFrames), st.nFrames);
    uint32_t flags = 0;

    DcsRunCursor runs;
    uint32_t poolUse = 0;               // counts every frame in full
    const DcsSlot empty{ 0xFFFFFFFFu, DCS_NO_PREV_SLOT, DCS_SLOT_EMPTY, 0, 0, 0, DCS_PREV_NONE, 0, 0, 0, 0, 0, 0, 0 };
    for (int p = 0 ; p < FPW ; ++p)
    {
        const uint32_t j = j0 + static_cast<uint32_t>(p);
        if (j >= nJobs || static_cast<uint32_t>(p) >= fpc) { out[p] = empty; continue; }
        while (k + 1 < nStreams && j >= streams[k + 1].firstJob)
        {
            ++k;
            st = streams[k];
            nValid = dcsMin(static_cast<uint32_t>(infos[k].nValidFrames), st.nFrames);
        }
        const uint32_t f = j - st.firstJob, framesOut = st.nFrames + extraFrames;
        const bool has = f < nValid;
        if (f == 0)
        {
            // (what counts is the bits the frames occupy, not nBytes, which includes the reference reader's look-ahead)
            const DcsStreamInfo in = infos[k];
            if (in.nFrames == 0 || 2u + static_cast<uint32_t>(in.hdrLen) + (in.payloadBits + 7) / 8 > st.len)
                flags |= DCS_PLAN_TRUNCATED;
        }
        DcsSlot sl{ j, DCS_NO_PREV_SLOT, 0, static_cast<uint8_t>(has ? 1 : 0),
                    static_cast<uint8_t>((has ? (f == 0 ? st.volShift0 : st.volShiftN) : 8) | (st.xform << 4)),
                    has ? st.firstRecord + f : 0u, f == 0 ? DCS_PREV_NONE : j - 1, 0, 0, 0, 0, 0, 0, 0 };
        if (f != 0)
        {
            if (p != 0)
                sl.prevSlot = static_cast<uint8_t>(p - 1);
            else
            {
                sl.flags |= DCS_SLOT_IMPORT;            // the chunk before publishes the tail (its last frame is this one's predecessor)
                sl.prevJob = c - 1;
            }
        }
        if ((static_cast<uint32_t>(p) == fpc - 1 || j + 1 == nJobs) && f + 1 < framesOut && j + 1 < nJobs)
        {
            sl.flags |= DCS_SLOT_EXPORT;
            sl.nextJob = j + 1;                     // (the stream's next frame: the first job of the next chunk)
        }
        if (f + 1 == framesOut)
            sl.flags |= DCS_SLOT_KEEP_TAIL;         // the last frame of its chain (dcs_plan.cpp)
        if (has)
        {
            const DcsRecDword *rec = reinterpret_cast<const DcsRecDword *>(&records[st.firstRecord + f]);
            const uint32_t bitOff = rec[0], nBits = rec[1] & 0xFFFFu, nBands = (rec[6] >> 16) & 0xFFu, fl = rec[6] >> 24;
            sl.bpl = dcsBandsPerLane(nBands, fl, FPW);
            const uint32_t n = dcsPoolDwords(st.streamOff, st.hdrLen, bitOff, nBits);
            sl.poolOff = static_cast<uint16_t>(runs.place(dcsFrameFirstDword(st.streamOff, st.hdrLen, bitOff), n));
            poolUse += (n + 3) & ~3u;
            srcs[st.firstRecord + f] = DcsPlanSrc{ st.streamOff, bitOff, static_cast<uint16_t>(nBits), st.hdrLen, static_cast<uint8_t>(nBands),
                                                   static_cast<uint8_t>(fl), st.format, f == 0 ? st.mixMul0 : st.mixMulN, st.firstRecord + f };
        }
        out[p] = sl;
        if (has)
            for (int r = 0 ; r <= p ; ++r)                  // slot k carries run k (constant subscripts: the slots stay in registers)
                if (static_cast<uint32_t>(r) + 1 == runs.nRuns)
                    runs.store(out[r]);
    }
    if (poolUse > dcsPoolCapacity(FPW) || runs.use > dcsPoolCapacity(FPW))
        flags |= DCS_PLAN_POOL_OVERFLOW;
    return flags;
}
#endif
