// dcs_encode93_rd.h -- constants, tables and records of the rate-distortion OS93 Type-0 encoder; the
// kernels are in dcs_encode93_rd.hip.h, which dcs_encode.hip includes behind every other kernel so that those keep their
// place in the code object.  The ladder, the quantiser's tables (EncRdTabs) and the bounds are dcs_encode_rd.h's.

namespace {

// the mixing multiplier the search reconstructs at: OS93a's as DESIGN.md 10.10 takes it (0x7FFF << 1), OS93b's what
// dcs_stream_params gives at volume, level and channel volume 0xFF for every frame but a fresh decoder's first
constexpr uint32_t kRd93M0a = 0xFFFE, kRd93M0b = 0xFEFC;
// a band's options, the trellis's states: 0 the zero band (code 0 in sub-type 0), 1..15 direct at width c + 1, then the
// delta and the double-delta coding of the unclamped values, then code 0 in sub-type 2 at (P, Dl) = (0, 0), which decodes
// to zeros: reached from the frame's start state and from itself alone
constexpr int kRd93States = 19, kRd93Delta = 16, kRd93DDelta = 17, kRd93Hold = 18;
constexpr uint32_t kRd93ItemsPerFrame = 16 * 64 * 16;           // [band][scale code][option] u64: D (option 0: the band's energy)
constexpr uint32_t kRd93RecsPerFrame = 16 * 64;                 // [band][scale code]
constexpr uint32_t kRd93ProxyPerJob = 16 * 64 * kRdKL;          // [band][scale code][lambda]
constexpr uint32_t kRd93MaxFrameBits = 16 * (1 + 6 + 16 * 16);  // every band: a 0 reuse bit, a sub-type change, 16 bits a value
constexpr uint32_t kRd93ChunkFrames = 64;                       // job-frames a block of the proxy and trellis kernels walks

// what the delta options need of a band's unclamped values at one scale code: the first two, the last two, and the signed
// widths of the first differences j = 1..15 and of the second differences j = 2..15
struct Enc93RdRec { int16_t q0, q1, q14, q15; uint8_t l1, l2, pad[2]; };
struct Enc93RdHead { uint8_t hv[16]; int32_t numBands; };       // per (job, lambda): the header vector the proxy chose
struct Enc93RdTot { unsigned long long D, bits; };              // per (job, lambda): the exact trellises' totals over the frames
struct Enc93RdChoice { int32_t ladderIndex, numBands, fits, pad; unsigned long long frameBits, sumD; uint8_t hv[16]; };
static_assert(sizeof(Enc93RdRec) == 12 && sizeof(Enc93RdHead) == 20 && sizeof(Enc93RdTot) == 16 && sizeof(Enc93RdChoice) == 48,
              "Enc93Rd records");

EncRdTabs buildTabs93Rd(uint32_t m0)
{
    EncRdTabs t = encTabsRd();                  // the ladder
    for (int j = 0 ; j < 64 ; ++j)
    {
        const unsigned long long s = kScaleMant[j & 3] >> (15 - (j >> 2));
        t.rcp[j] = static_cast<uint32_t>((1ull << 40) / (s * (m0 + 1)));
        t.qmax[j] = static_cast<int32_t>(32767 / s);
    }
    return t;
}

uint32_t rd93M0(uint16_t formatVersion) { return formatVersion == 0x9301 ? kRd93M0a : kRd93M0b; }

const EncRdTabs &encTabs93Rd(uint16_t formatVersion)
{
    static const EncRdTabs a = buildTabs93Rd(kRd93M0a), b = buildTabs93Rd(kRd93M0b);
    return formatVersion == 0x9301 ? a : b;
}

// E_b of one maximumQuantizationError, every band sixteen samples: min(floor(((K^2 q) q) 16), 2^40), compared in double
unsigned long long floorE93Rd(float maxQE)
{
    const double q = static_cast<double>(maxQE);
    const double e = floor(((1073741824.0 * q) * q) * 16.0);
    return e >= static_cast<double>(kRdFloorMax) ? kRdFloorMax : static_cast<unsigned long long>(e);
}

bool paramsValid93Rd(const DcsEncodeParams *p)
{
    return p != nullptr && (p->formatVersion == 0x9301 || p->formatVersion == 0x9302)
        && (p->streamFormatType == 0 || p->streamFormatType == -1) && p->targetBitRate >= 1 && p->targetBitRate <= 100000000
        && isfinite(p->powerBandCutoff) && isfinite(p->minimumDynamicRange) && isfinite(p->maximumQuantizationError);
}

}  // namespace
