// dcs_flac_walk_san.cpp -- the FLAC reader's walk on the host, for a sanitizer (tools/flac_walk_sanitize.sh builds it with
// -fsanitize=address,undefined on the host side and runs it where it was built; it calls no HIP API and is never run on a GPU).
//
//   dcs_flac_walk_san <pack>       pack: u32 count, then per file u64 bytes and the file (tests/flac_fuzz_cases.py --pack)
//
// Every file goes through flacParse in a heap copy of exactly its own length, so that a read past the file is a report.  A file
// the host accepts then takes the device's path with the host instantiations of the same routines (flacWalkFrame,
// flacRestoreChannel, flacUndoAssignment and flacCut are __host__ __device__), in buffers sized exactly as flacStage sizes the
// device's: the blob of every frame span rounded up to 256 bytes, plus 256; one int32 of staging per value; two descriptors
// a frame; the restore's history and taps as the kernel's LDS columns, 32 words 64 apart.  So a write past a frame's block, a
// descriptor index, a history slot or a shift count the format does not bound is a report here before it is a fault there.
//
// What the host cannot run is the device's form of FlacBits::load32: an aligned dword load that may begin up to 3 bytes
// before the frame's first subframe byte and end up to 3 bytes past the frame.  It never starts at or beyond `end`, so it
// stays inside [blob, blob + blobBytes + 3]; the program asserts that bound for every frame against the blob's size, whose
// 256 spare bytes flacStage allocates (held.alloc(&dBlob, blobBytes + 256), each allocation its own 256-aligned buffer).
//
// Output: one line per file, "<index> <status> <first error word or -> <checksum of the integers>".
#include "../../dcsexplorer_amd/csrc/dcs_encode.hip"

#include <memory>

namespace {

struct Result
{
    DcsStatus status;
    uint32_t err;           // frame << 4 | code, 0xFFFFFFFF: none
    uint64_t sum;
};

Result runFile(const uint8_t *file, uint64_t len)
{
    Result r{ DCS_OK, 0xFFFFFFFFu, 0 };
    DcsFlacInfo w;
    std::vector<DcsFlacFrame> ff;
    r.status = flacParse(file, len, &w, &ff);
    if (r.status != DCS_OK)
        return r;
    // flacStage's layout for a call of this one file
    const uint64_t span = ff.back().offset + ff.back().length - ff.front().offset;
    const uint64_t blobBytes = (span + 255) & ~uint64_t(255), blobAlloc = blobBytes + 256;
    std::unique_ptr<uint8_t[]> blob(new uint8_t[blobAlloc]);
    memcpy(blob.get(), file + ff.front().offset, span);
    memset(blob.get() + span, 0xA5, blobAlloc - span);
    const uint64_t nStage = w.nValues;
    std::unique_ptr<int32_t[]> stage(new int32_t[nStage]());
    std::unique_ptr<FlacSub[]> subs(new FlacSub[2 * ff.size()]());
    std::unique_ptr<int32_t[]> hist(new int32_t[32 * 64]()), taps(new int32_t[32 * 64]());
    for (uint64_t i = 0 ; i < ff.size() ; ++i)
    {
        const uint64_t byteOff = ff[i].offset - ff.front().offset, stageOff = ff[i].firstSample * static_cast<uint64_t>(w.channels);
        const uint8_t *first = blob.get() + byteOff;
        // the device's dword loads: from (first + hdrLen) rounded down to 4, to the dword holding the last byte before `end`
        const uint64_t endOff = byteOff + ff[i].length - 2;
        if (endOff > byteOff + static_cast<uint64_t>(ff[i].headerLength) && ((endOff - 1) | 3) >= blobAlloc)
        {
            fprintf(stderr, "frame %llu: the device's last dword would leave the blob\n", static_cast<unsigned long long>(i));
            abort();
        }
        if (stageOff + static_cast<uint64_t>(w.channels) * ff[i].blockSize > nStage)
        {
            fprintf(stderr, "frame %llu: its block would leave the staging buffer\n", static_cast<unsigned long long>(i));
            abort();
        }
        FlacBits br;
        br.init(first + ff[i].headerLength, first + ff[i].length - 2);
        uint32_t code = flacWalkFrame(br, ff[i].blockSize, w.channels, ff[i].channelAssignment, ff[i].bitsPerSample, stage.get() + stageOff,
                                      subs.get() + 2 * i);
        if (code == 0 && br.left != 0)
            code = kFlacErrLength;
        if (code != 0)
        {
            subs[2 * i].type = -1;
            subs[2 * i + 1].type = -1;
            r.err = std::min(r.err, static_cast<uint32_t>(i) << 4 | code);
            continue;
        }
        for (int32_t ch = 0 ; ch < w.channels ; ++ch)
            if (flacRestoreChannel(stage.get() + stageOff + static_cast<uint64_t>(ch) * ff[i].blockSize, ff[i].blockSize, subs[2 * i + ch],
                                   hist.get() + (i & 63), taps.get() + (i & 63), 64))
                r.err = std::min(r.err, static_cast<uint32_t>(i) << 4 | static_cast<uint32_t>(kFlacErrDepth));
    }
    // F3, whatever F1 and F2 flagged (the kernel runs over every frame too)
    for (uint64_t i = 0 ; i < ff.size() ; ++i)
    {
        const int32_t *s = stage.get() + ff[i].firstSample * static_cast<uint64_t>(w.channels);
        const uint32_t bs = ff[i].blockSize;
        for (uint32_t k = 0 ; k < bs ; ++k)
        {
            int32_t a = s[k], b = w.channels == 2 ? s[bs + k] : 0;
            if (w.channels == 2)
                flacUndoAssignment(ff[i].channelAssignment, a, b);
            const int32_t ca = w.sampleFormat == DCS_WAV_S8 ? flacCut<DCS_WAV_S8>(a) : w.sampleFormat == DCS_WAV_S16 ? flacCut<DCS_WAV_S16>(a) : flacCut<DCS_WAV_S24>(a);
            const int32_t cb = w.sampleFormat == DCS_WAV_S8 ? flacCut<DCS_WAV_S8>(b) : w.sampleFormat == DCS_WAV_S16 ? flacCut<DCS_WAV_S16>(b) : flacCut<DCS_WAV_S24>(b);
            r.sum = r.sum * 1000003u + static_cast<uint32_t>(ca) + 31u * static_cast<uint32_t>(cb);
        }
    }
    return r;
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
    uint32_t count = 0;
    if (f == nullptr || fread(&count, 4, 1, f) != 1)
    {
        fprintf(stderr, "usage: dcs_flac_walk_san <pack>\n");
        return 2;
    }
    uint32_t accepted = 0, host = 0, device = 0;
    for (uint32_t i = 0 ; i < count ; ++i)
    {
        uint64_t len;
        if (fread(&len, 8, 1, f) != 1)
            return 2;
        std::unique_ptr<uint8_t[]> data(new uint8_t[len]);      // exactly the file: a read past it is a report
        if (len != 0 && fread(data.get(), 1, len, f) != len)
            return 2;
        const Result r = runFile(data.get(), len);
        if (r.status != DCS_OK) ++host; else if (r.err != 0xFFFFFFFFu) ++device; else ++accepted;
        if (r.err == 0xFFFFFFFFu)
            printf("%u %d - %016llx\n", i, static_cast<int>(r.status), static_cast<unsigned long long>(r.sum));
        else
            printf("%u %d %u:%u %016llx\n", i, static_cast<int>(r.status), r.err >> 4, r.err & 15u, static_cast<unsigned long long>(r.sum));
    }
    fclose(f);
    fprintf(stderr, "%u files: %u accepted, %u refused by the host index, %u refused by the walk or the restore\n", count, accepted, host, device);
    return 0;
}
