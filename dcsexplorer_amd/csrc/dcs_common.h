// dcs_common.h -- internal declarations shared by the host side and the HIP kernels of libdcs_hip.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "../../include/dcs_hip.h"

// ---------------------------------------------------------------------------------------------
// Decode tables as the kernels consume them.  Built once on the host from the canonical code lists
// in dcs_tables.h (dcs_tables.cpp), uploaded at context creation, and staged into LDS by every
// workgroup (the `lds` part) or read through L1/L2 (the rest).
//
// Variable-length codes are decoded with a 256-entry first-level table on the next 8 bits plus a
// binary trie for the (rare) longer codes:
//   fast[peek8]  : bit15 set  -> leaf:  bits 11..8 = code length (1..8), bits 7..0 = payload
//                  bit15 clear -> index of the trie node reached after those 8 bits
//   trie[n]      : bit15 set  -> leaf payload (bits 7..0); clear -> index of the '0' child, the
//                  '1' child is the next entry
// Payload for the 1994+ band-type deltas is delta+16 (0..30); for the 1993b band types it is the
// raw 6-bit leaf value of the format (<0x1E: keep sub-type, value-0x0F; else toggle, value-0x2E).
// ---------------------------------------------------------------------------------------------
#define DCS_CB94_TOTAL   940            // 4+8+32+128+256+512 direct-lookup entries, codebooks 1..6
#define DCS_TRIE94_MAX   64
#define DCS_TRIE93_MAX   128

struct DcsLdsTables
{
    // ---- what the decode kernel stages (the first DCS_LDS_DECODE_BYTES) -----------------------------------------------
    uint16_t cb94[DCS_CB94_TOTAL];      // entry = sample (signed byte, 0 for the two-zeros code) | nBits<<8 | step<<13
                                        // (step = samples the code stands for: 1, or 2 for two zeros; .cpp:2046-2175)
    uint16_t fast93[256];
    uint16_t trie93[DCS_TRIE93_MAX];
    uint16_t bandBits93a[64];           // bandBits (0xFF = end of frame) | prefixBits<<8 (:2878-2902)
    uint16_t scaleCb93a[80];            // value (0xFF = escape) | nBits<<8 | subTable<<12 (:2938-2959)
    uint8_t  inputs93a[24];             // inputs per band, 18 used (:2865)
    uint16_t raw94[20];                 // two-entry "codebooks" of the fixed-width sample codes 7..16: width<<8 | 1<<13
    // Everything the 1994+ band set-up derives from a band-type code (:1886-2005), resolved once (dcs_tables.cpp) so that
    // the kernel's set-up is one look-up: [0..50] Type 1, [band class 0..2][min(code, 16)]; [51..68] Type 0, [min(code, 17)].
    // Entry: the codebook's offset in this block, in half-words (bits 0..10) | 32 - look-ahead width (11..15) | shift
    // that turns the next 32 bits into the codebook index (16..20) | DCS_B94_RAW | _ZERO | _STOP | _FATAL | scale
    // adjustment << 25.
    uint32_t band94[72];
    uint16_t scale64[64];               // scale factor of a band by the low six bits of its scale code (:1978-1979, :2342)
    uint8_t  padDecode_[8];
    // ---- the index walk only (dcs_scan.h; the index kernel stages the whole block) ---------------------------------------
    uint16_t cbInfo[8];                 // per sample code 1..6: maxBits | (base offset into cb94)<<4
    uint16_t xlat94[48];                // [band class 0..2][code] = typeCode | scalingAdj<<8 (:1926-1953)
    uint8_t  preAdj94[32];              // [0..15] sub-type 0 map, [16..31] sub-type 1..3 map (:1744-1749)
    uint16_t scaleMant[4];              // 0x8000, 0x9838, 0xB505, 0xD745 (:1978)
    uint8_t  pad_[8];
};
// (gfx950 hands LDS out in 1 280-byte pieces: with 16 frames per wavefront a workgroup's 4 x 12 576 bytes leave 3 456
// for the tables if three workgroups are to share a CU)
#define DCS_LDS_DECODE_BYTES 3424
#define DCS_B94_RAW      (1u << 21)     // fixed-width samples (sample codes 7..16)
#define DCS_B94_ZERO     (1u << 22)     // nothing coded (:1886)
#define DCS_B94_STOP     (1u << 23)     // sample code 0 behind a non-zero band-type code (:1985-1991)
#define DCS_B94_FATAL    (1u << 24)     // no such code (:1914, :1999)
#define DCS_B94_TYPE0    51             // first Type-0 entry

// per-lane constants of the transform passes (dcs_kernels.hip.h): twiddles and overlap-window entries that
// depend only on the lane number, precomputed on the host so that a wavefront fetches them with six
// 16-byte loads per lane instead of ~40 scattered table reads.  One 24-dword record per transform:
//   1994+ (lane94[l], l = lane & 7 matters):  [0..7]  pre-twiddle of pair i = l + 8j: c0 | c1 << 16 (.cpp:428-429)
//                                             [8..21] layout-B stages d=4 [8..9], d=2 [10..13], d=1 [14..21]; cos | sin << 16
//                                             [22]    overlap window of pair m = bitrev3(l): co[2m] | co[2m+1] << 16
//                                             [23]    co[15-2m] | co[14-2m] << 16
//   1993  (lane93[l], l = lane & 15 matters): [0..14] layout-B stages d=8 [0], d=4 [1..2], d=2 [3..6], d=1 [7..14]
//                                             [15]    overlap window of sample i = bitrev4(l): co[i] | co[15-i] << 16
#define DCS_LANE_CONSTS 24
#define DCS_K94_PRE   0
#define DCS_K94_TWB   8
#define DCS_K94_OVLA  22
#define DCS_K94_OVLB  23
#define DCS_K93_TWB   0
#define DCS_K93_OVL   15

struct DcsDevTables
{
    DcsLdsTables lds;                   // copied to LDS by each workgroup
    uint32_t lane94[64][DCS_LANE_CONSTS];
    uint32_t lane93[64][DCS_LANE_CONSTS];
    uint16_t fast94[256];               // 1994+ band-type delta code: only the host index pass reads it
    uint16_t trie94[DCS_TRIE94_MAX];
    uint16_t pair93a[2048];             // OS93a Type-1 sample pair table (:2698-2827); read via L1/L2
    uint16_t fftCoef[256];              // sin block 0..0x7F, cos block 0x80..0xFF, bit-reversed order (:366)
    uint16_t ovlCoef[16];               // overlap window (:314)
    int32_t  twA[8][4];                 // twiddles 0..7 as the in-lane (layout A) butterflies take them: 2 cos, 2 sin, -2 sin, 0
    // The device index pass (dcs_index_wave.hip.h) takes several 1994+ sample codes per step: per codebook 1..6 and for the
    // next DCS_IDX_MULTI_BITS bits, the codes that lie entirely inside them, as long as they stand for at most
    // DCS_IDX_MULTI_SAMPLES samples together (at least one code): total length | samples << 4
    uint8_t  multi94[6][1 << 10];
    // The band plan of the decode kernel (planBand94, dcs_kernels.hip.h; 8 frames per wavefront, which stage it into LDS): what a
    // band's record takes from its band-type code alone, [strided][key of lds.band94] -> two dwords,
    //   [0] codebook's offset in the lds block in bytes (bits 0..15) | scale adjustment (16..22) | bytes of tile row per sample
    //       of the band, halved count: 2, 4 for a coded strided band, 0 for a code that is none (24..26)
    //   [1] the record's second dword but for its last byte
    uint32_t plan94[2][72][2];
};
#define DCS_PLAN94_BYTES 1152
#define DCS_IDX_MULTI_BITS 10
#define DCS_IDX_MULTI_SAMPLES 4

// host-side view (same structure; one process-wide immutable instance)
const DcsDevTables &dcsTables();

// MainLoop's shared fixed-point scale with a per-channel master multiplier (dcs_params.cpp)
int dcsFrameScaleV(const uint16_t *vol, uint16_t *mixMul, const uint8_t *counted, int nch);

// the kernel work list (DcsSlot), the chunk plan's rules and the chunk packages
#include "dcs_package.h"

struct DcsKernelArgs
{
    const uint8_t      *blob;
    uint64_t            blobLen;        // bytes that may be read (allocation is padded beyond this)
    const DcsSrcDesc   *srcs;
    uint8_t            *packages;       // nChunks x dcsPkgStride(fpw, layout), see above
    uint32_t            nChunks;
    uint32_t            nJobs;
    int16_t            *pcm;            // nJobs x 240
    uint32_t           *err;            // nJobs
    const int16_t      *tailsIn;        // k x 16 (may be null)
    int16_t            *tailsOut;       // nJobs x 16 (may be null)
    const DcsDevTables *tables;
    unsigned long long *debug;          // diagnostic builds only (DCS_STAMPS); null otherwise
    // tails between chunks (the rendezvous, dcs_kernels.hip.h): nChunks x 16 words of epoch << 33 | who << 32 | payload; a word
    // belongs to this launch when its epoch equals `epoch` (the launch counter, 1 .. 2^31 - 1), so the buffer is never cleared
    unsigned long long *handoff;
    uint32_t            epoch;
    uint32_t            flags;          // DCS_BATCH_*
};
#define DCS_EPOCH_MAX 0x7FFFFFFFu
#define DCS_BATCH_HAS_93A_T1 1u         // some source is an OS93a Type-1 frame: workgroups stage the pair table in LDS
// The chunks are in CHAIN order (a chunk takes its tail from the chunk before it) and the launch maps them to workgroups in XCD
// RANGES: workgroup i of a launch runs on XCD i % 8 (measured: tools/xcd_map.hip), so with logical workgroup
// L = (i % 8) * R + i / 8, R = workgroups / 8, XCD j decodes logical workgroups [j R, (j + 1) R) in order, and the producer of a tail
// sits in the same workgroup or in the one dispatched just before it ON THE SAME XCD.  Every wait is then for a wavefront that is
// resident or through whatever else runs on the chip -- other decode kernels included (dcs_pipeline.hip.h: why that matters); only
// the first workgroup of a range may wait for the last one of the range before, i.e. until that XCD is through.
#define DCS_BATCH_XCD_RANGES 2u
// set by the launch, not by the batch: more than one wavefront per SIMD, so the wavefronts arrange their priorities (s_setprio,
// dcs_kernels.hip.h); bits 8..15 then hold CUs / 8 (CUs x 4 workgroups are resident at once)
#define DCS_BATCH_PACED 4u
#define DCS_BATCH_CUS8_SHIFT 8
// the packages deal 1994+ frames to their eight unpack lanes in units of 8 samples (dcs_package.h: the even deal), and the symbol
// loop runs in rounds of 8 samples (8 frames per wavefront, first source)
#define DCS_BATCH_EVEN_DEAL 8u
// no job of the batch has a second source (classifyJobs): with the even deal, the launch may take the kernels without the rounds of
// further sources (dcsDecodeKernel<8, CPW, true, true>; dcs_ctx_set_sole_source_kernel)
#define DCS_BATCH_SOLE_SOURCE 16u
// bits 5..7: 16 less the most header bands any 1994+ first source of the batch fills tile words for, at most 7 (createBatch, for
// batches that may take those kernels; 0: all sixteen, or not recorded).  Behind word 16 (nb - 1) - 1 of every row of the batch
// nothing is ever written, and the 1994+ transform's pre-pass leaves out the partners that lie there (dcsPrepassShort,
// dcs_package.h; transform94x8).  A source whose split or mid records start a lane later than the library's own walk would --
// caller-made records may -- counts as sixteen bands.
#define DCS_BATCH_BANDS_SHIFT 5
#define DCS_BATCH_BANDS_MASK  7u
#define DCS_BATCH_IMG_SHIFT 16          // bits 16..31: the packages' layout word (image dwords | DCS_PKG_SPLIT4; dcsPkgStride)
#define DCS_BATCH_IMG_MASK  0xFFFFu

// what the index kernel writes per frame next to the full record: all the host needs for planning (8 bytes)
struct DcsFrameDigest
{
    uint32_t bitOff;
    uint16_t nBits;
    uint8_t  nBands, flags;
};

#ifdef __cplusplus
#include <vector>
// whole streams -> batch description (dcs_streams.cpp): index pass on the host pool, per-frame mixing parameters, the
// streams laid out back to back in one blob, one job per output frame
struct DcsBuiltStreams
{
    std::vector<uint8_t> blob;
    std::vector<DcsSrcDesc> srcs;
    std::vector<DcsFrameJob> jobs;
    std::vector<uint32_t> firstJob;     // per stream, plus a final total
};
// index records made elsewhere (the device index pass) for streams already laid out in a blob of the caller's: the build
// then neither walks the streams nor copies them (B.blob stays empty; sources point into the caller's blob)
struct DcsPreIndexed
{
    const DcsFrameIndex *records;       // stream k's records at records + firstRecord[k]
    const uint64_t *firstRecord;
    const DcsStreamInfo *infos;
    const uint64_t *streamOff;          // stream k's offset in the caller's blob; NULL: the build lays the streams out itself
};
DcsStatus dcsBuildStreams(const DcsStreamRef *streams, uint32_t nStreams, uint32_t extraFrames, DcsBuiltStreams &B,
                          bool countOnly, bool sequence, const DcsPreIndexed *pre = nullptr);
// The same batch description in its light form, for packing on the device: jobs as above, sources as 24-byte
// digests (DcsPlanSrc) that name their index record by position (`recordBase` + the stream's first record + frame).
struct DcsDigested
{
    const DcsFrameDigest *digest;       // stream k's frames at digest + firstRecord[k]
    const uint64_t *firstRecord;
    const DcsStreamInfo *infos;
    const uint64_t *streamOff;          // stream k's offset in the uploaded blob
    uint32_t recordBase;                // where this list's records start in the device-resident record array
};
#include <functional>
DcsStatus dcsIndexStreamsNotify(const DcsStreamRef *streams, uint32_t nStreams, int nThreads,
                                DcsFrameIndex *out, const uint64_t *firstRecord, DcsStreamInfo *infos, DcsFrameMids *mids,
                                const std::function<void(uint32_t)> *done);
bool dcsIndexPoolBusy();
void dcsHostPoolRun(uint32_t n, int threads, const std::function<void(uint32_t)> &fn);
// the host walk with its records handed over frame by frame, and the container part of it alone (dcs_index.cpp)
DcsStatus dcsIndexStreamProgressive(DcsOsVersion os, const uint8_t *stream, size_t len, DcsStreamInfo *info,
                                    const std::function<void(uint32_t, const DcsFrameIndex &)> &onFrame);
DcsStatus dcsStreamContainer(DcsOsVersion os, const uint8_t *stream, size_t len, DcsStreamInfo *info);
// large lists through the context's own pipeline, in parts (dcs_large_list.hip.h); *handled = false: take the direct path
DcsStatus dcsDecodeStreamsInParts(DcsCtx *ctx, const DcsStreamRef *streams, uint32_t nStreams, uint32_t extraFrames,
                                  int16_t *pcmOut, size_t pcmCapFrames, uint32_t *frameOffsets, uint32_t *errOut, bool *handled);
struct DcsBuiltPlan
{
    std::vector<DcsFrameJob> jobs;
    std::vector<DcsPlanSrc> srcs;
    std::vector<uint32_t> firstJob;
};
DcsStatus dcsBuildPlanFromDigest(const DcsStreamRef *streams, uint32_t nStreams, uint32_t extraFrames, const DcsDigested &in,
                                 DcsBuiltPlan &P);
// every source the jobs draw on is a 1994+ frame (the packages then carry 4-byte split records, DCS_PKG_SPLIT4)
bool dcsAllSources94(const DcsFrameJob *jobs, uint32_t nJobs, const DcsSrcDesc *srcs);
// The planner (dcs_plan.cpp), from either form of source record.  slots is resized to nChunks x fpw; imgDw: dwords of pool image
// the packages of the plan need -- the fullest chunk's runs, rounded up to 32 dwords, at most the pool's capacity.
struct DcsPlanOptions
{
    bool handoff = true;                // tails between chunks go through the hand-off buffer (else every chunk re-decodes a halo)
    int framesPerChunk = 0;             // diagnostic: fewer frames per chunk than the kernel variant has slots (0: all of them)
    bool keepAllTails = false;          // every frame's slot gets DCS_SLOT_KEEP_TAIL, else only the last frame of every chain
    uint32_t places = 0;                // a RESIDENT batch: wavefronts of the decode kernel the chip runs at a time (CUs x 16); the plan
                                        // is then made a second time for the shortest packages (dcs_plan.cpp).  0: planned once
};
struct DcsPlan { uint32_t nChunks, imgDw; };
DcsPlan dcsPlanJobs(const DcsFrameJob *jobs, uint32_t nJobs, const DcsSrcDesc *srcs, int fpw, std::vector<DcsSlot> &slots, const DcsPlanOptions &o);
DcsPlan dcsPlanJobs(const DcsFrameJob *jobs, uint32_t nJobs, const DcsPlanSrc *srcs, int fpw, std::vector<DcsSlot> &slots, const DcsPlanOptions &o);
// (a test hook: the chunks in a seeded random order -- the rendezvous between chunks must not care; seed 0: as planned)
void dcsShuffleChunks(std::vector<DcsSlot> &slots, uint32_t nChunks, int fpw, uint32_t seed);
#define DCS_MI355X_WAVE_PLACES 4096u    // (the diagnostic entries assume an MI355X)
// packer: out = nChunks x dcsPkgStride(fpw, layout) bytes (the chunk packages described above); layout = image dwords | DCS_PKG_SPLIT4
// mids: the sources' mid records, parallel to srcs, for a batch that takes the even deal (DCS_BATCH_EVEN_DEAL); null: whole bands
void dcsBuildPackages(const DcsSlot *slots, uint32_t nChunks, int fpw, const DcsSrcDesc *srcs,
                      const uint8_t *blob, size_t blobLen, uint8_t *out, uint32_t layout, const DcsFrameMids *mids = nullptr);
// what the even deal saves the fullest unpack lane of a frame of nb header bands, in samples, against whole bands (8 lanes)
int dcsEvenDealGain(int nb);
#endif
