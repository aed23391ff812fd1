// dcs_plan_test -- the arithmetic planner of a list of whole streams (dcsPlanChunk, dcs_package.h: the body of the device
// planner, callable on the host) against the chain planner (dcsPlanJobs over DcsPlanSrc digests): every slot field the packer or
// the decode kernel reads, and the source digests.  Needs no GPU.  Prints one line per failure; exit status 0 = all equal.
#include "../../dcsexplorer_amd/csrc/dcs_common.h"
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
static size_t slotsCompared = 0, plansCompared = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 40) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } } while (0)

static std::vector<uint8_t> synth(int format, int nFrames, uint64_t seed, int profile)
{
    DcsSynthParams p;
    memset(&p, 0, sizeof p);
    p.seed = seed; p.format = format; p.nFrames = nFrames; p.nBands = format == DCS_FMT_93A_T1 ? 18 : 16; p.strideFromBand = 16; p.profile = profile;
    size_t n = 0;
    dcs_synth_stream(&p, nullptr, 0, &n);
    std::vector<uint8_t> s(n);
    if (dcs_synth_stream(&p, s.data(), n, &n) != DCS_OK)
        s.clear();
    return s;
}
static int osOf(int format, int k)
{
    return format == DCS_FMT_93A_T1 ? DCS_OS93A : format == DCS_FMT_93B_T1 ? DCS_OS93B : format == DCS_FMT_93_T0 ? ((k & 1) ? DCS_OS93A : DCS_OS93B)
                                                                                                              : ((k & 1) ? DCS_OS95 : DCS_OS94);
}

// a list of whole streams, indexed on the host and laid out in a blob, and the arithmetic planner's stream table for it
struct List
{
    std::vector<std::vector<uint8_t>> data;
    std::vector<DcsStreamRef> refs;
    std::vector<uint64_t> firstRecord, streamOff;
    std::vector<DcsFrameIndex> records;
    std::vector<DcsStreamInfo> infos;
    void add(std::vector<uint8_t> s, int os) { data.push_back(std::move(s)); refs.push_back(DcsStreamRef{ nullptr, 0, os, 230, 0x60 + static_cast<int>(refs.size() % 5), 255 }); }
    bool index()
    {
        uint64_t nRec = 0, off = 0;
        for (size_t k = 0 ; k < refs.size() ; ++k)
        {
            refs[k].data = data[k].data();
            if (refs[k].len == 0)
                refs[k].len = data[k].size();       // (set beforehand: a stream handed over short of its payload)
            firstRecord.push_back(nRec);
            streamOff.push_back(off);
            nRec += (static_cast<uint32_t>(data[k][0]) << 8) | data[k][1];
            off += (refs[k].len + 3) & ~size_t(3);
        }
        records.assign(nRec, DcsFrameIndex{});
        infos.assign(refs.size(), DcsStreamInfo{});
        return dcs_index_streams(refs.data(), static_cast<uint32_t>(refs.size()), 1, records.data(), firstRecord.data(), infos.data()) == DCS_OK;
    }
    // (what planTableFor, dcs_plan_device.hip.h, makes from the streams' first bytes; here from the index pass's summary)
    bool table(uint32_t extraFrames, std::vector<DcsPlanStream> &t, uint32_t &nJobs) const
    {
        nJobs = 0;
        t.assign(refs.size(), DcsPlanStream{});
        for (size_t k = 0 ; k < refs.size() ; ++k)
        {
            const DcsOsVersion os = static_cast<DcsOsVersion>(refs[k].os);
            uint16_t mm[2]; uint8_t vs[2];
            if (dcs_stream_params_from(os, refs[k].volume, refs[k].level, refs[k].channelVolume, 0x7FFF, 2, mm, vs) != DCS_OK)
                return false;
            t[k].streamOff = streamOff[k];
            t[k].len = static_cast<uint32_t>(refs[k].len);
            t[k].firstRecord = static_cast<uint32_t>(firstRecord[k]);
            t[k].firstJob = nJobs;
            t[k].nFrames = (static_cast<uint32_t>(data[k][0]) << 8) | data[k][1];
            t[k].mixMul0 = mm[0]; t[k].mixMulN = mm[1]; t[k].volShift0 = vs[0]; t[k].volShiftN = vs[1];
            t[k].xform = (os == DCS_OS93A || os == DCS_OS93B) ? DCS_XFORM_93 : DCS_XFORM_94;
            t[k].hdrLen = static_cast<uint8_t>(infos[k].hdrLen);
            t[k].format = static_cast<uint8_t>(infos[k].format);
            nJobs += t[k].nFrames + extraFrames;
        }
        return true;
    }
};

template <int FPW>
static uint32_t planArithmetic(const List &l, const std::vector<DcsPlanStream> &t, uint32_t extraFrames, uint32_t nJobs, uint32_t fpc,
                               std::vector<DcsSlot> &slots, std::vector<DcsPlanSrc> &srcs)
{
    const uint32_t nChunks = (nJobs + fpc - 1) / fpc;
    slots.assign(static_cast<size_t>(nChunks) * FPW, DcsSlot{});
    srcs.assign(l.records.size(), DcsPlanSrc{});
    uint32_t flags = 0;
    for (uint32_t c = 0 ; c < nChunks ; ++c)
        flags |= dcsPlanChunk<FPW>(t.data(), static_cast<uint32_t>(t.size()), l.infos.data(), l.records.data(), extraFrames, nJobs, fpc, c,
                                   &slots[static_cast<size_t>(c) * FPW], srcs.data());
    return flags;
}

template <int FPW>
static void compare(const List &l, uint32_t extraFrames, int framesPerChunk)
{
    char what[64];
    snprintf(what, sizeof what, "fpw %d extra %u fpc %d", FPW, extraFrames, framesPerChunk);
    std::vector<DcsPlanStream> t;
    uint32_t nJobs = 0;
    if (!l.table(extraFrames, t, nJobs)) { CHECK(false, "%s: stream table", what); return; }
    std::vector<DcsSlot> arith;
    std::vector<DcsPlanSrc> arithSrcs;
    const uint32_t fpc = static_cast<uint32_t>(framesPerChunk > 0 ? framesPerChunk : FPW);
    const uint32_t flags = planArithmetic<FPW>(l, t, extraFrames, nJobs, fpc, arith, arithSrcs);
    CHECK(flags == 0, "%s: the arithmetic planner raised flags %u", what, flags);

    // the chain planner's input: the job list of the same records, its sources as digests numbered like the records
    DcsBuiltStreams B;
    const DcsPreIndexed pre{ l.records.data(), l.firstRecord.data(), l.infos.data(), l.streamOff.data() };
    if (dcsBuildStreams(l.refs.data(), static_cast<uint32_t>(l.refs.size()), extraFrames, B, false, false, &pre) != DCS_OK || B.jobs.size() != nJobs)
    {
        CHECK(false, "%s: dcsBuildStreams", what);
        return;
    }
    std::vector<DcsPlanSrc> digests(l.records.size(), DcsPlanSrc{});
    for (size_t k = 0, j = 0 ; k < l.refs.size() ; ++k)
        for (uint32_t f = 0 ; f < t[k].nFrames + extraFrames ; ++f, ++j)
            if (B.jobs[j].nSrc != 0)
            {
                const DcsSrcDesc &sd = B.srcs[B.jobs[j].firstSrc];
                const uint32_t record = t[k].firstRecord + f;
                digests[record] = DcsPlanSrc{ sd.streamOff, sd.idx.bitOff, sd.idx.nBits, sd.hdrLen, sd.idx.nBands, sd.idx.flags, sd.format, sd.mixMul, record };
                B.jobs[j].firstSrc = record;
            }
    std::vector<DcsSlot> chain;
    DcsPlanOptions o;
    o.framesPerChunk = framesPerChunk;
    const DcsPlan plan = dcsPlanJobs(B.jobs.data(), nJobs, digests.data(), FPW, chain, o);
    CHECK(plan.nChunks * static_cast<size_t>(FPW) == arith.size(), "%s: %u chunks, arithmetic %zu", what, plan.nChunks, arith.size() / FPW);
    if (chain.size() != arith.size())
        return;
    ++plansCompared;
    slotsCompared += chain.size();
    for (size_t i = 0 ; i < chain.size() ; ++i)
    {
        const DcsSlot &a = chain[i], &b = arith[i];
#define SAME(field) CHECK(a.field == b.field, "%s: chunk %zu slot %zu: " #field " %u, arithmetic %u", what, i / FPW, i % FPW, unsigned(a.field), unsigned(b.field))
        SAME(job); SAME(prevSlot); SAME(flags); SAME(nSrc); SAME(shiftXform); SAME(prevJob);
        SAME(runStartDw); SAME(runNDw); SAME(runPoolOff); SAME(poolOff); SAME(bpl);
        if (a.nSrc != 0)
            SAME(firstSrc);
        if (a.flags & DCS_SLOT_EXPORT)
            SAME(nextJob);
#undef SAME
    }
    CHECK(memcmp(digests.data(), arithSrcs.data(), sizeof(DcsPlanSrc) * digests.size()) == 0, "%s: the source digests differ", what);
}

// flip payload bits until the index pass stops the stream early (nValidFrames < nFrames)
static std::vector<uint8_t> damaged(int format, int nFrames, uint64_t seed)
{
    const std::vector<uint8_t> good = synth(format, nFrames, seed, 0);
    uint64_t x = seed;
    for (int attempt = 0 ; attempt < 4000 && good.size() > 40 ; ++attempt)
    {
        std::vector<uint8_t> s = good;
        for (int k = 0 ; k < 3 ; ++k)
        {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            s[18 + (x >> 33) % (s.size() / 2 - 18)] ^= static_cast<uint8_t>(1u << ((x >> 20) & 7));
        }
        DcsStreamInfo info;
        if (dcs_index_stream(DCS_OS94, s.data(), s.size(), nullptr, 0, &info) != DCS_ERR_INVALID_ARG && info.nValidFrames < info.nFrames)
            return s;
    }
    return {};
}

template <int FPW>
static void run(int smallerFpc)
{
    const int lengths[6] = { 1, 2, FPW - 1, FPW, FPW + 1, 37 };
    List l;
    for (int i = 0 ; i < 36 ; ++i)
    {
        const int format = i % 6, nFrames = lengths[(i / 6 + i) % 6];       // every layout at every length, mixed
        l.add(synth(format, nFrames, 0x9400 + 64 * FPW + i, i % 3), osOf(format, i));
        if (i == 17)
            l.add(damaged(DCS_FMT_94_T1_S3, 37, 0xDA3A6ED + FPW), DCS_OS94);
    }
    for (const std::vector<uint8_t> &s : l.data)
        if (s.size() < 4) { CHECK(false, "fpw %d: no stream (synth, or no damage that stops the index pass)", FPW); return; }
    if (!l.index()) { CHECK(false, "fpw %d: index pass", FPW); return; }
    CHECK(l.infos[18].nValidFrames < l.infos[18].nFrames, "fpw %d: the damaged stream indexed whole", FPW);
    for (uint32_t extra = 0 ; extra <= 2 ; ++extra)
        for (int fpc : { 0, smallerFpc })
            compare<FPW>(l, extra, fpc);

    // a stream handed over short of its payload: the arithmetic plan must say so (the list then takes the chain planner's path)
    List cut;
    cut.add(synth(DCS_FMT_94_T1_S3, 37, 0xC07 + FPW, 0), DCS_OS94);
    cut.add(synth(DCS_FMT_93B_T1, FPW + 1, 0xC08 + FPW, 0), DCS_OS93B);
    cut.refs[0].len = cut.data[0].size() / 2;
    std::vector<DcsPlanStream> t;
    uint32_t nJobs = 0;
    if (!cut.index() || !cut.table(1, t, nJobs)) { CHECK(false, "fpw %d: the cut list", FPW); return; }
    std::vector<DcsSlot> slots;
    std::vector<DcsPlanSrc> srcs;
    const uint32_t flags = planArithmetic<FPW>(cut, t, 1, nJobs, FPW, slots, srcs);
    CHECK((flags & DCS_PLAN_TRUNCATED) != 0, "fpw %d: a stream cut short of its payload raised flags %u", FPW, flags);
}

int main()
{
    run<4>(3);
    run<8>(6);
    run<16>(12);
    if (failures == 0)
        printf("dcs_plan_test: the arithmetic planner and the chain planner agree on %zu slots of %zu plans\n", slotsCompared, plansCompared);
    else
        printf("dcs_plan_test: %d failures\n", failures);
    return failures == 0 ? 0 : 1;
}
