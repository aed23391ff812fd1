// dcs_encode_rd.h -- constants, tables and records of the rate-distortion 1994+ encoder; the kernels are
// in dcs_encode_rd.hip.h, which dcs_encode.hip includes behind every other kernel so that those keep their place in the
// code object.

namespace {

constexpr int kRdKL = 56;                          // the ladder's entries
constexpr int kRdNH = 14, kRdHStep = 3;            // header scale codes searched per band, this far apart
constexpr int kRdHBase0 = 2, kRdHBase1 = 21;       // ... downwards from this far below the band's top code (Type 0, Type 1)
constexpr uint32_t kRdM0 = 0xFEFC;                 // the 1994+ mixing multiplier at volume, level and channel volume 0xFF
constexpr float kRdK = 32768.0f;
constexpr unsigned long long kRdInf = 1ull << 62;  // no path; every real cost is below 2^58
constexpr unsigned long long kRdFloorMax = 1ull << 40;
constexpr unsigned long long kRdNoItem = ~0ull;
constexpr unsigned long long kRdDMask = (1ull << 48) - 1;       // an item: D in the low 48 bits, the sample bits above
constexpr uint32_t kRdRowsPerLayout = 16 * kRdNH * kRdKL;
constexpr uint32_t kRdRowsPerJob = 3 * kRdRowsPerLayout;
constexpr uint32_t kRdItemsPerFrame = 16 * 16 * 64;
static_assert(kRdRowsPerLayout % 16 == 0, "a block of sixteen rows is of one layout");

struct EncRdTabs
{
    unsigned long long ladder[kRdKL];
    uint32_t rcp[64];                  // floor(2^40 / (scale * (M0 + 1))): the quantiser's estimate
    int32_t qmax[64];                  // floor(32767 / scale): |q * scale| stays in 16 bits signed
};

EncRdTabs buildTabsRd()
{
    EncRdTabs t;
    memset(&t, 0, sizeof(t));
    t.ladder[0] = 0;
    t.ladder[1] = 1;
    for (int k = 0 ; k < kRdKL - 3 ; ++k)
        t.ladder[k + 2] = static_cast<unsigned long long>(2 + (k & 1)) << (k >> 1);
    t.ladder[kRdKL - 1] = 1ull << 32;
    for (int j = 0 ; j < 64 ; ++j)
    {
        const unsigned long long s = kScaleMant[j & 3] >> (15 - (j >> 2));
        t.rcp[j] = static_cast<uint32_t>((1ull << 40) / (s * (kRdM0 + 1)));
        t.qmax[j] = static_cast<int32_t>(32767 / s);
    }
    return t;
}

const EncRdTabs &encTabsRd() { static const EncRdTabs t = buildTabsRd(); return t; }

// every frame at the widest option: each band behind the longest delta code, at width 15
uint32_t rdMaxFrameBits()
{
    uint32_t longest = 0, bits = 0;
    for (int i = 0 ; i < 31 ; ++i)
        longest = std::max<uint32_t>(longest, encTabs().hdrLen[i]);
    for (int b = 0 ; b < 16 ; ++b)
        bits += longest + 15u * kBandCount94[b];
    return bits;
}

// E_b of one maximumQuantizationError: min(floor(((K^2 q) q) count_b), 2^40), compared in double before the cast
void floorERd(float maxQE, unsigned long long *row)
{
    const double q = static_cast<double>(maxQE);
    for (int b = 0 ; b < 16 ; ++b)
    {
        const double e = floor(((1073741824.0 * q) * q) * static_cast<double>(kBandCount94[b]));
        row[b] = e >= static_cast<double>(kRdFloorMax) ? kRdFloorMax : static_cast<unsigned long long>(e);
    }
}

struct EncRdTot { unsigned long long J, D; uint32_t bits, pad; };
struct EncRdChoice { int32_t variant, ladderIndex, numBands, fits; unsigned long long frameBits, sumD; uint8_t hk[16]; };
static_assert(sizeof(EncRdTot) == 24 && sizeof(EncRdChoice) == 48, "EncRd records");

bool paramsValidRd(const DcsEncodeParams *p)
{
    return p != nullptr && p->formatVersion == 0x9400 && p->streamFormatType >= -1 && p->streamFormatType <= 1
        && (p->streamFormatSubType == -1 || p->streamFormatSubType == 0 || p->streamFormatSubType == 3)
        && p->targetBitRate >= 1 && p->targetBitRate <= 100000000
        && isfinite(p->powerBandCutoff) && isfinite(p->minimumDynamicRange) && isfinite(p->maximumQuantizationError);
}

}  // namespace
