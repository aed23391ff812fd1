// dcs_wav.hip.h -- the reference's EncodeFile on files held in memory (DCSEncodeFile.cpp:29-105): a "DCSa" container goes
// through transcoding (EncodeDCSFile), a RIFF/WAVE file is read as libnyquist's WavDecoder::LoadFromBuffer reads it
// (WavDecoder.cpp, Common.cpp ReadFile / ConvertToFloat32, Common.h ScanForChunk and the *_to_float32 macros), downmixed,
// resampled and encoded.  Included at the end of dcs_encode.hip, after dcs_resample.hip.h: it shares that translation unit's
// floating-point contract (no contraction; the divisions by 32767, 2^23 and 2^31 are correctly rounded divisions).
//
//   W0 ima     wavImaKernel          one lane per (IMA ADPCM block, channel): the block's nibbles, serially, to int16 at
//                                    libnyquist's offsets in a staging buffer
//   W1 unpack  wavUnpackKernel<F>    one thread per mono sample: the raw payload (or W0's int16) converted as libnyquist
//                                    converts it, the stereo mean (L + R) / 2.0f; a non-finite value flags its file.  Its
//                                    output is the staged mono buffer the resampler's walk (R2) and convolution (R3) read.
//
// The host parses each file (dcs_wav_parse), and only the `data` payloads go up.  The walk is routed by size (rsHostRoute).
#pragma once

namespace {

const uint32_t kWavGuidTail[3] = { 0x00100000u, 0xAA000080u, 0x719B3800u };     // KSDATAFORMAT_SUBTYPE_*: bytes 4..15

uint32_t rd32(const uint8_t *p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24; }
uint16_t rd16(const uint8_t *p) { return static_cast<uint16_t>(p[0] | p[1] << 8); }
uint32_t fourcc(const char *s) { return rd32(reinterpret_cast<const uint8_t *>(s)); }

// ScanForChunk (Common.h): the first 2-byte-aligned occurrence of the code anywhere in the file, payloads included; offset 0
// means none.  The reference reads the code and the size past the end of the buffer near its end: a match whose 8 bytes do
// not all lie in the file is no match here (INTEGRATION.md "Encoding files", rule 8).
struct WavChunk { uint64_t offset, size; };
WavChunk wavScan(const uint8_t *f, uint64_t len, uint32_t code)
{
    for (uint64_t i = 0 ; 2 * i + 8 <= len ; ++i)
        if (rd32(f + 2 * i) == code)
            return WavChunk{ 2 * i, rd32(f + 2 * i + 4) };
    return WavChunk{ 0, 0 };
}

int wavWidth(int32_t fmt)
{
    switch (fmt)
    {
        case DCS_WAV_U8: return 1;
        case DCS_WAV_S16: return 2;
        case DCS_WAV_S24: return 3;
        case DCS_WAV_S32: case DCS_WAV_F32: return 4;
        case DCS_WAV_F64: return 8;
        default: return 0;
    }
}

DcsStatus wavRefuse(DcsWavInfo *w, DcsStatus st, const char *why)
{
    snprintf(w->reason, sizeof(w->reason), "%s", why);
    return st;
}

// LoadFromBuffer's reading of one file, with the library's rules where the reference is undefined or departs from the format
DcsStatus wavParse(const uint8_t *f, uint64_t len, DcsWavInfo *w)
{
    memset(w, 0, sizeof(*w));
    if (len < 64)
        return wavRefuse(w, DCS_ERR_INVALID_ARG, "file too small (under 64 bytes)");
    if (len >= (uint64_t(1) << 32))
        return wavRefuse(w, DCS_ERR_INVALID_ARG, "4 GiB or more");
    const uint32_t id = rd32(f);
    if (id != fourcc("RIFF"))
        return wavRefuse(w, DCS_ERR_INVALID_ARG, id == fourcc("RIFX") || id == fourcc("FFIR") ? "big-endian RIFX file"
                                                                                               : "bad RIFF header");
    if (rd32(f + 8) != fourcc("WAVE"))
        return wavRefuse(w, DCS_ERR_INVALID_ARG, "bad WAVE header");
    if (uint64_t(rd32(f + 4)) + 8 != len)
        return wavRefuse(w, DCS_ERR_INVALID_ARG, "the RIFF size is not the file's length less 8");
    const WavChunk fmt = wavScan(f, len, fourcc("fmt "));
    if (fmt.offset == 0)
        return wavRefuse(w, DCS_ERR_INVALID_ARG, "no fmt chunk");
    if (fmt.offset + 24 > len)
        return wavRefuse(w, DCS_ERR_BAD_STREAM, "the fmt chunk runs past the end of the file");
    const uint8_t *h = f + fmt.offset;
    if (rd32(h + 4) < 16)
        return wavRefuse(w, DCS_ERR_INVALID_ARG, "fmt chunk smaller than 16 bytes");
    w->formatCode = rd16(h + 8);
    w->channels = rd16(h + 10);
    w->rate = rd32(h + 12);
    w->blockAlign = rd16(h + 20);
    w->bitDepth = rd16(h + 22);
    const int32_t bits = w->bitDepth;
    bool isFloat = w->formatCode == 3;
    if (w->formatCode == 0xFFFE)
    {
        // rule 10: the SubFormat GUID decides (libnyquist reads every EXTENSIBLE file as integer PCM)
        if (rd32(h + 4) < 40)
            return wavRefuse(w, DCS_ERR_INVALID_ARG, "WAVE_FORMAT_EXTENSIBLE with a fmt chunk shorter than 40 bytes");
        if (fmt.offset + 48 > len)
            return wavRefuse(w, DCS_ERR_BAD_STREAM, "the EXTENSIBLE fmt chunk runs past the end of the file");
        const uint8_t *g = h + 32;
        const uint32_t sub = rd32(g);
        if ((sub != 1 && sub != 3) || rd32(g + 4) != kWavGuidTail[0] || rd32(g + 8) != kWavGuidTail[1] || rd32(g + 12) != kWavGuidTail[2])
            return wavRefuse(w, DCS_ERR_INVALID_ARG, "WAVE_FORMAT_EXTENSIBLE with a sub-format other than PCM or IEEE float");
        isFloat = sub == 3;
        if (isFloat && bits != 32 && bits != 64)
            return wavRefuse(w, DCS_ERR_INVALID_ARG, "IEEE float samples of other than 32 or 64 bits");
    }
    else if (w->formatCode != 1 && w->formatCode != 3 && w->formatCode != 0x11)
        return wavRefuse(w, DCS_ERR_INVALID_ARG, "format code other than PCM (1), IEEE float (3), IMA ADPCM (0x11), EXTENSIBLE (0xFFFE)");
    const bool ima = w->formatCode == 0x11;
    if (ima)
    {
        if (bits != 4)
            return wavRefuse(w, DCS_ERR_INVALID_ARG, "IMA ADPCM of other than 4 bits");
        w->sampleFormat = DCS_WAV_IMA;
    }
    else
        switch (bits)           // LoadFromBuffer's switch; 64-bit integers and the other depths have no conversion
        {
            case 4: case 16: w->sampleFormat = DCS_WAV_S16; break;
            case 8: w->sampleFormat = DCS_WAV_U8; break;
            case 24: w->sampleFormat = DCS_WAV_S24; break;
            case 32: w->sampleFormat = isFloat ? DCS_WAV_F32 : DCS_WAV_S32; break;
            case 64:
                if (!isFloat)
                    return wavRefuse(w, DCS_ERR_INVALID_ARG, "64-bit integer samples (libnyquist does not convert them)");
                w->sampleFormat = DCS_WAV_F64;
                break;
            default:
                return wavRefuse(w, DCS_ERR_INVALID_ARG, "a bit depth libnyquist does not convert");
        }
    if (w->channels != 1 && w->channels != 2)
        return wavRefuse(w, DCS_ERR_INVALID_ARG, "channel count other than 1 or 2");
    const WavChunk data = wavScan(f, len, fourcc("data"));
    if (data.offset == 0)
        return wavRefuse(w, DCS_ERR_INVALID_ARG, "no data chunk");
    w->dataOffset = data.offset + 8;
    w->dataSize = data.size;
    if (w->dataOffset + w->dataSize > len)
        return wavRefuse(w, DCS_ERR_BAD_STREAM, "the data chunk runs past the end of the file");
    if (w->blockAlign == 0)
        return wavRefuse(w, DCS_ERR_BAD_STREAM, "block align 0 (the reference divides by it)");
    const uint64_t C = static_cast<uint64_t>(w->channels), fs = static_cast<uint64_t>(w->blockAlign);
    if (!ima)
    {
        w->nValues = (w->dataSize / fs) * C;
        if (w->dataOffset + w->nValues * wavWidth(w->sampleFormat) > len)
            return wavRefuse(w, DCS_ERR_BAD_STREAM, "the samples run past the end of the file (block align too small)");
        return DCS_OK;
    }
    // IMA ADPCM: fact.sample_length * channels values are kept (u32 arithmetic, as the reference computes it)
    const WavChunk fact = wavScan(f, len, fourcc("fact"));
    if (fact.size == 0)
        return wavRefuse(w, DCS_ERR_BAD_STREAM, "IMA ADPCM without a fact chunk (the reference reads an uninitialised count)");
    if (fact.offset + 12 > len)
        return wavRefuse(w, DCS_ERR_BAD_STREAM, "the fact chunk runs past the end of the file");
    const uint32_t total = rd32(f + fact.offset + 8) * static_cast<uint32_t>(C);
    if (fs < 4 * C || (fs - 4 * C) % (4 * C) != 0)
        return wavRefuse(w, DCS_ERR_INVALID_ARG, "IMA ADPCM block align that is not 4 x channels x (1 + a whole number of words)");
    w->nValues = total;
    w->nBlocks = w->dataSize / fs;
    if (w->nBlocks * (2 * fs - 8 * C) > 2 * uint64_t(total))
        return wavRefuse(w, DCS_ERR_BAD_STREAM, "IMA ADPCM blocks that would write past twice the fact chunk's count");
    for (uint64_t b = 0 ; b < w->nBlocks ; ++b)
        for (uint64_t c = 0 ; c < C ; ++c)
        {
            const uint8_t *hdr = f + w->dataOffset + b * fs + 4 * c;
            if (hdr[3] != 0)
                return wavRefuse(w, DCS_ERR_BAD_STREAM, "IMA ADPCM block header with a nonzero reserved byte");
            if (hdr[2] > 88)
                return wavRefuse(w, DCS_ERR_BAD_STREAM, "IMA ADPCM block header with a step index above 88");
        }
    return DCS_OK;
}

// ------------------------------------------------------------------------------------------------------------- kernels

__constant__ int32_t kWavImaStep[89] = {
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130,
    143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282,
    1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630,
    9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767 };

// what one WAV file is on the device
struct WavFile
{
    uint64_t payOff;        // the payload's first byte in the uploaded blob (256-byte aligned); IMA: W0's first int16
    uint64_t nValues;       // values libnyquist produces (interleaved)
    uint64_t monoOff;       // first mono sample in the staged buffer
    uint64_t nMono;
    uint64_t blobOff;       // IMA: the payload's first byte in the blob
    uint32_t nBlocks;       // IMA: whole blocks
    int32_t blockAlign;
    int32_t channels;
    int32_t sampleFormat;   // DCS_WAV_*
};

// decode_nibble (WavDecoder.cpp): int16_t p += diff wraps modulo 2^16 (x86 g++), so the clamp after it never acts
__device__ inline int16_t wavImaNibble(uint32_t n, int32_t &p, int32_t &s)
{
    const int32_t step = kWavImaStep[s];
    int32_t diff = step >> 3;
    if (n & 4) diff += step;
    if (n & 2) diff += step >> 1;
    if (n & 1) diff += step >> 2;
    if (n & 8) diff = -diff;
    p = static_cast<int16_t>(p + diff);
    s += (n & 7) < 4 ? -1 : 2 * static_cast<int32_t>((n & 7) - 3);          // ima_index_table
    s = s < 0 ? 0 : s > 88 ? 88 : s;
    return static_cast<int16_t>(p);
}

// W0: blockIdx.y strides over the IMA files (`which`), x over a file's (block, channel) lanes.  Block b's values start at
// b * (2 * blockAlign - 8 * channels); only the first nValues are kept (the host checked that the blocks fit in twice that).
__global__ __launch_bounds__(64) void wavImaKernel(const uint8_t *__restrict__ blob, const WavFile *__restrict__ files,
                                                   const uint32_t *__restrict__ which, uint32_t nWhich, int16_t *__restrict__ staged)
{
    for (uint32_t wi = blockIdx.y ; wi < nWhich ; wi += gridDim.y)
    {
        const WavFile w = files[which[wi]];
        const uint32_t C = static_cast<uint32_t>(w.channels), fs = static_cast<uint32_t>(w.blockAlign);
        for (uint64_t lane = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x ; lane < uint64_t(w.nBlocks) * C
             ; lane += uint64_t(gridDim.x) * blockDim.x)
        {
            const uint32_t b = static_cast<uint32_t>(lane / C), c = static_cast<uint32_t>(lane % C);
            const uint8_t *data = blob + w.blobOff + uint64_t(b) * fs;
            int16_t *out = staged + w.payOff;
            const uint64_t base = uint64_t(b) * (2 * fs - 8 * C);
            int32_t p = static_cast<int16_t>((data[4 * c + 1] << 8) | data[4 * c]), s = data[4 * c + 2];
            uint64_t idx = c;
            for (uint32_t byteIdx = 4 * C + 4 * c ; byteIdx < fs ; byteIdx += 4 * (C - 1))
                for (int j = 0 ; j < 4 ; ++j, ++byteIdx)
                {
                    const uint32_t v = data[byteIdx];
                    const int16_t lo = wavImaNibble(v & 15u, p, s);
                    if (base + idx < w.nValues)
                        out[base + idx] = lo;
                    idx += C;
                    const int16_t hi = wavImaNibble(v >> 4, p, s);
                    if (base + idx < w.nValues)
                        out[base + idx] = hi;
                    idx += C;
                }
        }
    }
}

// the *_to_float32 macros (Common.h) on an integer already read, bit for bit; shared with F3 (dcs_flac.hip.h)
template <int F>
__device__ inline float wavScale(int32_t x)
{
    if constexpr (F == DCS_WAV_U8)
        return (static_cast<float>(x) - 128) * (1.0f / 127.0f);
    else if constexpr (F == DCS_WAV_S8)
        return static_cast<float>(x) * (1.0f / 127.0f);
    else if constexpr (F == DCS_WAV_S16 || F == DCS_WAV_IMA)
        return static_cast<float>(x) / 32767.f;
    else if constexpr (F == DCS_WAV_S24)
        return static_cast<float>(x) / 8388608.f;
    else
        return static_cast<float>(x) / 2147483648.f;
}

// EncodeFile's downmix of a stereo pair (DCSEncodeFile.cpp)
__device__ inline float wavMean(float l, float r) { return (l + r) / 2.0f; }

// ConvertToFloat32 (Common.cpp), bit for bit
template <int F>
__device__ inline float wavValue(const uint8_t *__restrict__ p, const int16_t *__restrict__ ima, uint64_t k)
{
    if constexpr (F == DCS_WAV_U8)
        return wavScale<F>(p[k]);
    else if constexpr (F == DCS_WAV_S16)
        return wavScale<F>(reinterpret_cast<const int16_t *>(p)[k]);
    else if constexpr (F == DCS_WAV_IMA)
        return wavScale<F>(ima[k]);
    else if constexpr (F == DCS_WAV_S24)
    {
        const uint8_t *q = p + 3 * k;
        const int32_t x = (static_cast<int32_t>(static_cast<int8_t>(q[2])) << 16) | (q[1] << 8) | q[0];
        return wavScale<F>(x);
    }
    else if constexpr (F == DCS_WAV_S32)
        return wavScale<F>(reinterpret_cast<const int32_t *>(p)[k]);
    else if constexpr (F == DCS_WAV_F32)
        return reinterpret_cast<const float *>(p)[k];
    else
        return static_cast<float>(reinterpret_cast<const double *>(p)[k]);
}

// W1: blockIdx.y strides over the files of format F (`which`), x over a file's mono samples
template <int F>
__global__ __launch_bounds__(256) void wavUnpackKernel(const uint8_t *__restrict__ blob, const int16_t *__restrict__ staged,
                                                       const WavFile *__restrict__ files, const uint32_t *__restrict__ which,
                                                       uint32_t nWhich, float *__restrict__ mono, uint32_t *__restrict__ bad)
{
    for (uint32_t wi = blockIdx.y ; wi < nWhich ; wi += gridDim.y)
    {
        const uint32_t fi = which[wi];
        const WavFile &w = files[fi];
        const uint8_t *p = blob + w.payOff;
        const int16_t *q = staged + w.payOff;
        const bool stereo = w.channels == 2;
        bool isBad = false;
        for (uint64_t j = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x ; j < w.nMono ; j += uint64_t(gridDim.x) * blockDim.x)
        {
            float x;
            if (stereo && 2 * j + 1 < w.nValues)
                x = wavMean(wavValue<F>(p, q, 2 * j), wavValue<F>(p, q, 2 * j + 1));
            else
                x = wavValue<F>(p, q, stereo ? 2 * j : j);
            if (!isfinite(x))
                isBad = true;
            mono[w.monoOff + j] = x;
        }
        if (isBad)
            atomicOr(&bad[fi], 1u);
    }
}

// ----------------------------------------------------------------------------------------------------------- host side

// A FLAC file among the files of a call (dcs_flac.hip.h, included after this file): its record and frame index; both null
// for a WAV file.  Its DcsWavInfo is flacAsWav's.
struct FlacSource
{
    const DcsFlacInfo *info;
    const std::vector<DcsFlacFrame> *frames;
};
DcsStatus flacStage(DcsCtx *ctx, CacheArena &held, hipStream_t st, const uint8_t *const *bytes, const FlacSource *flac, uint32_t n,
                    const std::vector<WavFile> &wf, float *dMono, std::vector<uint32_t> &errOut);
DcsStatus flacParse(const uint8_t *f, uint64_t len, DcsFlacInfo *w, std::vector<DcsFlacFrame> *frames);
DcsWavInfo flacAsWav(const DcsFlacInfo &w);
bool isFlacFile(const uint8_t *f, uint64_t len);
std::string stageWhy(uint32_t bad);

// The parsed WAV and FLAC files of one call on the device: payloads up, W0, W1; frames up, F1, F2, F3 (flac null: no FLAC
// file).  On DCS_OK *dMono holds file k's mono samples from files[k].monoOff; bad[k] is set where a value or a pair's mean is
// not finite, or (top bit) where a FLAC frame is refused on the device: stageWhy says which.  Buffers belong to `held`.
DcsStatus wavStageOnDevice(DcsCtx *ctx, const uint8_t *const *bytes, const DcsWavInfo *infos, const FlacSource *flac, uint32_t n,
                           std::vector<WavFile> &wf, CacheArena &held, float **dMonoOut, std::vector<uint32_t> &bad)
{
    const auto isFlac = [&](uint32_t k) { return flac != nullptr && flac[k].info != nullptr; };
    bool anyFlac = false;
    wf.assign(n, WavFile{});
    uint64_t blobBytes = 0, nStaged = 0, nMono = 0, maxMono = 0, maxLanes = 0;
    std::vector<uint32_t> byFormat[DCS_WAV_IMA + 1];
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const DcsWavInfo &w = infos[k];
        WavFile &f = wf[k];
        const bool ima = w.sampleFormat == DCS_WAV_IMA;
        const uint64_t payload = isFlac(k) ? 0 : ima ? w.nBlocks * static_cast<uint64_t>(w.blockAlign) : w.nValues * wavWidth(w.sampleFormat);
        f.blobOff = blobBytes;
        f.payOff = ima ? nStaged : blobBytes;
        blobBytes += (payload + 255) & ~uint64_t(255);
        nStaged += ima ? w.nValues : 0;
        f.nValues = w.nValues;
        f.nMono = rsMonoLength(w.nValues, w.channels);
        f.monoOff = nMono;
        f.nBlocks = static_cast<uint32_t>(w.nBlocks);
        f.blockAlign = w.blockAlign;
        f.channels = w.channels;
        f.sampleFormat = w.sampleFormat;
        nMono += f.nMono;
        maxMono = f.nMono > maxMono ? f.nMono : maxMono;
        if (ima)
            maxLanes = w.nBlocks * w.channels > maxLanes ? w.nBlocks * w.channels : maxLanes;
        if (isFlac(k))
            anyFlac = true;
        else
            byFormat[w.sampleFormat].push_back(k);
    }
    const hipStream_t st = dcsCtxStream(ctx);
    uint8_t *dBlob;
    int16_t *dStaged;
    float *dMono;
    WavFile *dFiles;
    uint32_t *dWhich, *dBad;
    ENCCHK(hipSetDevice(dcsCtxDevice(ctx)));
    ENCCHK(held.alloc(&dBlob, blobBytes ? blobBytes : 1));
    ENCCHK(held.alloc(&dStaged, nStaged ? nStaged : 1));
    ENCCHK(held.alloc(&dMono, nMono ? nMono : 1));
    ENCCHK(held.alloc(&dFiles, n));
    ENCCHK(held.alloc(&dWhich, n));
    ENCCHK(held.alloc(&dBad, n));
    for (uint32_t k = 0 ; k < n ; ++k)
    {
        const DcsWavInfo &w = infos[k];
        const uint64_t payload = w.sampleFormat == DCS_WAV_IMA ? w.nBlocks * static_cast<uint64_t>(w.blockAlign)
                                                               : w.nValues * wavWidth(w.sampleFormat);
        if (payload != 0 && !isFlac(k))
            ENCCHK(hipMemcpyAsync(dBlob + wf[k].blobOff, bytes[k] + w.dataOffset, payload, hipMemcpyHostToDevice, st));
    }
    std::vector<uint32_t> which;
    std::vector<size_t> whichOff(DCS_WAV_IMA + 2, 0);
    for (int fmt = 0 ; fmt <= DCS_WAV_IMA ; ++fmt)
    {
        whichOff[fmt] = which.size();
        which.insert(which.end(), byFormat[fmt].begin(), byFormat[fmt].end());
    }
    whichOff[DCS_WAV_IMA + 1] = which.size();
    ENCCHK(hipMemcpyAsync(dFiles, wf.data(), sizeof(WavFile) * n, hipMemcpyHostToDevice, st));
    if (!which.empty())
        ENCCHK(hipMemcpyAsync(dWhich, which.data(), sizeof(uint32_t) * which.size(), hipMemcpyHostToDevice, st));
    ENCCHK(hipMemsetAsync(dBad, 0, sizeof(uint32_t) * n, st));
    const uint32_t nIma = static_cast<uint32_t>(byFormat[DCS_WAV_IMA].size());
    if (nIma != 0)
    {
        // the values no block writes stay zero, as in the reference's zero-filled vector
        ENCCHK(hipMemsetAsync(dStaged, 0, sizeof(int16_t) * nStaged, st));
        if (maxLanes != 0)
        {
            const uint64_t lb = (maxLanes + 63) / 64;
            hipLaunchKernelGGL(wavImaKernel, dim3(static_cast<unsigned>(lb < 65535 ? lb : 65535), nIma < 65535 ? nIma : 65535), dim3(64),
                               0, st, dBlob, dFiles, dWhich + whichOff[DCS_WAV_IMA], nIma, dStaged);
        }
    }
    const uint64_t blocks = (maxMono + 255) / 256;
    const unsigned gx = static_cast<unsigned>(blocks < 1 ? 1 : blocks < 1024 ? blocks : 1024);
    for (int fmt = 0 ; fmt <= DCS_WAV_IMA ; ++fmt)
    {
        const uint32_t m = static_cast<uint32_t>(byFormat[fmt].size());
        if (m == 0)
            continue;
        const dim3 grid(gx, m < 65535 ? m : 65535);
        const uint32_t *w = dWhich + whichOff[fmt];
        switch (fmt)
        {
            case DCS_WAV_U8: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_U8>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            case DCS_WAV_S16: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_S16>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            case DCS_WAV_S24: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_S24>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            case DCS_WAV_S32: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_S32>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            case DCS_WAV_F32: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_F32>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            case DCS_WAV_F64: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_F64>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
            default: hipLaunchKernelGGL(wavUnpackKernel<DCS_WAV_IMA>, grid, dim3(256), 0, st, dBlob, dStaged, dFiles, w, m, dMono, dBad); break;
        }
    }
    ENCCHK(hipGetLastError());
    std::vector<uint32_t> flacErr;
    if (anyFlac)
        ENCTRY(flacStage(ctx, held, st, bytes, flac, n, wf, dMono, flacErr));
    bad.assign(n, 0);
    ENCCHK(hipMemcpyAsync(bad.data(), dBad, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    ENCCHK(hipStreamSynchronize(st));
    for (uint32_t k = 0 ; anyFlac && k < n ; ++k)
        if (flacErr[k] != 0xFFFFFFFFu)
            bad[k] = 0x80000000u | flacErr[k];
    *dMonoOut = dMono;
    return DCS_OK;
}

bool isDcsaFile(const uint8_t *f, uint64_t len)          // DCSEncoder::IsDCSFile (DCSEncoder.cpp:381-386)
{
    return len >= 36 && memcmp(f, "DCSa", 4) == 0 && (f[4] == 0x93 || f[4] == 0x94) && f[6] == 0 && f[7] == 1 && f[8] == 0x7A
           && f[9] == 0x12;
}

bool isRiffFile(const uint8_t *f, uint64_t len)
{
    return len >= 4 && (memcmp(f, "RIFF", 4) == 0 || memcmp(f, "RIFX", 4) == 0 || memcmp(f, "FFIR", 4) == 0);
}

// "stream <k>" at the start of a message from a sub-call -> "file <map[k]>" (map null: "file <k>")
void renameError(DcsCtx *ctx, const std::vector<uint32_t> *map)
{
    const std::string msg = dcs_last_error(ctx);
    if (msg.compare(0, 7, "stream ") != 0)
        return;
    size_t end = 7;
    uint64_t k = 0;
    while (end < msg.size() && msg[end] >= '0' && msg[end] <= '9')
        k = k * 10 + static_cast<uint64_t>(msg[end++] - '0');
    if (end == 7 || (map != nullptr && k >= map->size()))
        return;
    dcsCtxSetError(ctx, ("file " + std::to_string(map != nullptr ? (*map)[k] : k) + msg.substr(end)).c_str());
}

// INTEGRATION rule 12: the largest |x| the encoder accepts from a file, the most negative value of its source format as
// libnyquist converts it: -32768 / 32767 for 16-bit PCM, ADPCM and FLAC, (0 - 128) / 127 for u8 and -128 / 127 for FLAC's
// signed 8 bits (rule 25); 1 for the others
float wavBound(int32_t fmt)
{
    if (fmt == DCS_WAV_S16 || fmt == DCS_WAV_IMA)
        return 32768.0f / 32767.0f;
    if (fmt == DCS_WAV_U8 || fmt == DCS_WAV_S8)
        return 128.0f / 127.0f;
    return 1.0f;
}

// What the plan knows of one file without a GPU
struct FilePlan
{
    int32_t kind = -1;
    DcsStatus status = DCS_OK;
    std::string why;
    DcsWavInfo wav{};               // (a FLAC file's is flacAsWav's)
    DcsFlacInfo flac{};
    std::vector<DcsFlacFrame> flacFrames;
    DcsStreamRef ref{};
    uint64_t bound = 0;
};

void flacParseMany(const uint8_t *files, const uint64_t *fileOffsets, const std::vector<uint32_t> &which, std::vector<FilePlan> &plan);

// The length limit, checked before anything is allocated: fewer than 2^31 mono samples (what the resampler's walk indexes,
// as rsCheck requires of the other entry points) and, for encoding (s given), a 31 250 Hz length the encoder's 65 535 frames
// can take.  The walk's exact count is known only after it runs, so a file is refused here when even its room less twice the
// filter's reach and the end-of-input flush exceeds 65 535 frames; nearer the limit the exact count decides after the walk.
bool wavLengthOk(const DcsWavInfo &w, const RsStream *s, std::string &why)
{
    const uint64_t m = rsMonoLength(w.nValues, w.channels), cap = uint64_t(65535) * 240;
    if (m >= (uint64_t(1) << 31))
    {
        why = "2^31 mono samples or more";
        return false;
    }
    if (s == nullptr)
        return true;
    const uint64_t reach = static_cast<uint64_t>(2.0 * static_cast<double>(s->half) / s->step) + kRsFlushCap + 8;
    const uint64_t room = s->passThrough ? m : rsSlots(*s);
    if (room > cap + reach)
    {
        why = "resamples to more than 65 535 frames";
        return false;
    }
    return true;
}

DcsStatus planFiles(const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles, const DcsEncodeParams *params,
                    const DcsResampleFilter &f, uint32_t flags, std::vector<FilePlan> &plan)
{
    plan.assign(nFiles, FilePlan{});
    const bool os93 = params->formatVersion != 0x9400;
    std::vector<uint32_t> flacIdx;
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        if (!isDcsaFile(files + fileOffsets[i], fileOffsets[i + 1] - fileOffsets[i]) && !isRiffFile(files + fileOffsets[i], fileOffsets[i + 1] - fileOffsets[i])
            && isFlacFile(files + fileOffsets[i], fileOffsets[i + 1] - fileOffsets[i]))
            flacIdx.push_back(i);
    if (!flacIdx.empty())
        flacParseMany(files, fileOffsets, flacIdx, plan);
    for (uint32_t i = 0 ; i < nFiles ; ++i)
    {
        FilePlan &p = plan[i];
        const std::string name = "file " + std::to_string(i);
        const uint8_t *b = files + fileOffsets[i];
        const uint64_t len = fileOffsets[i + 1] - fileOffsets[i];
        if (isDcsaFile(b, len))
        {
            DcsOsVersion os;
            const uint8_t *s;
            uint32_t nBytes;
            if (dcs_dcsa_parse(b, len, &os, &s, &nBytes) != DCS_OK)
            {
                p.status = DCS_ERR_BAD_STREAM;
                p.why = name + ": a DCSa container whose data size runs past the end of the file";
                continue;
            }
            p.ref = DcsStreamRef{ s, nBytes, os, 0x67, 0xFF, 0xFF };        // EncodeDCSFile's decode settings
            int32_t action;
            std::string why;
            p.status = dcsTranscodePlan(&p.ref, 1, params, 0, &action, &p.bound, why);
            if (p.status != DCS_OK)
            {
                p.why = why.compare(0, 9, "stream 0:") == 0 ? name + why.substr(8) : name + ": " + why;
                continue;
            }
            p.kind = action == DCS_TRANSCODE_COPIED ? DCS_FILE_DCSA_COPY : DCS_FILE_DCSA_REENCODE;
            continue;
        }
        const bool flac = !isRiffFile(b, len) && isFlacFile(b, len);
        if (flac)
        {
            if (p.status != DCS_OK)                         // (flacParseMany's)
            {
                p.why = name + ": " + p.flac.reason;
                continue;
            }
            p.wav = flacAsWav(p.flac);
        }
        else if (!isRiffFile(b, len))
        {
            p.status = DCS_ERR_INVALID_ARG;
            p.why = name + ": not a DCSa container, a RIFF/WAVE file or a FLAC file";
            continue;
        }
        else
        {
            p.status = wavParse(b, len, &p.wav);
            if (p.status != DCS_OK)
            {
                p.why = name + ": " + p.wav.reason;
                continue;
            }
        }
        const DcsWavInfo &w = p.wav;
        if (w.rate < kRsMinRate || w.rate > kRsMaxRate)
        {
            p.status = DCS_ERR_INVALID_ARG;
            p.why = name + ": rate " + std::to_string(w.rate) + " Hz is outside 4 000 .. 384 000";
            continue;
        }
        const uint64_t m = rsMonoLength(w.nValues, w.channels);
        if (m == 0)
        {
            p.status = DCS_ERR_INVALID_ARG;
            p.why = name + ": no samples";
            continue;
        }
        const RsStream s = rsStreamOf(m, w.rate, f, flags);
        if (!wavLengthOk(w, &s, p.why))
        {
            p.status = DCS_ERR_INVALID_ARG;
            p.why = name + ": " + p.why;
            continue;
        }
        p.kind = flac ? DCS_FILE_FLAC : DCS_FILE_WAV;
        const uint64_t count = s.passThrough ? m : rsSlots(s);
        const uint64_t cap = uint64_t(65535) * 240;
        p.bound = (os93 ? dcs_encode93_bound : dcs_encode_bound)(count < cap ? count : cap);
    }
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        if (plan[i].status != DCS_OK)
            return plan[i].status;
    return DCS_OK;
}

DcsStatus filesArgs(const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles, const DcsEncodeParams *params,
                    const DcsResampleFilter *filter, uint32_t flags, DcsResampleFilter &f, std::string &why)
{
    if (fileOffsets == nullptr || (nFiles != 0 && files == nullptr))
        return DCS_ERR_INVALID_ARG;
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        if (fileOffsets[i + 1] < fileOffsets[i])
            return DCS_ERR_INVALID_ARG;
    const bool os93 = params != nullptr && params->formatVersion != 0x9400;
    if (!paramsValid(params, os93))
    {
        if (const char *type1 = whyOs93aType1(params, os93))
            why = type1;
        return DCS_ERR_INVALID_ARG;
    }
    const uint64_t none[1] = { 0 };
    return rsCheck(0, none, nullptr, nullptr, filter, flags, f, why);
}

}  // namespace

extern "C" DcsStatus dcs_wav_parse(const uint8_t *file, size_t len, DcsWavInfo *info)
{
    if (info == nullptr || (file == nullptr && len != 0))
        return DCS_ERR_INVALID_ARG;
    DcsWavInfo w;
    const DcsStatus st = file == nullptr ? wavRefuse(&w, DCS_ERR_INVALID_ARG, "file too small (under 64 bytes)") : wavParse(file, len, &w);
    w.status = st;
    *info = w;
    return st;
}

extern "C" DcsStatus dcs_encode_files_plan(const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles,
                                           const DcsEncodeParams *params, const DcsResampleFilter *filter, uint32_t flags,
                                           int32_t *kindOut, uint64_t *boundOut, int32_t *statusOut)
{
    DcsResampleFilter f;
    std::string why;
    DcsStatus st = filesArgs(files, fileOffsets, nFiles, params, filter, flags, f, why);
    if (st != DCS_OK)
        return st;
    std::vector<FilePlan> plan;
    st = planFiles(files, fileOffsets, nFiles, params, f, flags, plan);
    for (uint32_t i = 0 ; i < nFiles ; ++i)
    {
        if (kindOut != nullptr) kindOut[i] = plan[i].kind;
        if (boundOut != nullptr) boundOut[i] = plan[i].bound;
        if (statusOut != nullptr) statusOut[i] = plan[i].status;
    }
    return st;
}

namespace {
// dcs_wav_decode (flac false) and dcs_flac_decode (true): each takes its own kind of file only
DcsStatus wavDecode(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles, float *out,
                                    size_t outCap, uint64_t *outOffsets, bool flac)
{
    if (ctx == nullptr || fileOffsets == nullptr || outOffsets == nullptr || (nFiles != 0 && files == nullptr))
        return DCS_ERR_INVALID_ARG;
    std::vector<DcsWavInfo> infos(nFiles);
    std::vector<const uint8_t *> bytes(nFiles);
    std::vector<DcsFlacInfo> flacInfos(flac ? nFiles : 0);
    std::vector<std::vector<DcsFlacFrame>> flacFrames(flac ? nFiles : 0);
    std::vector<FlacSource> sources(flac ? nFiles : 0);
    outOffsets[0] = 0;
    for (uint32_t i = 0 ; i < nFiles ; ++i)
    {
        if (fileOffsets[i + 1] < fileOffsets[i])
            return DCS_ERR_INVALID_ARG;
        bytes[i] = files + fileOffsets[i];
        DcsStatus st;
        std::string why;
        if (flac)
        {
            st = flacParse(bytes[i], fileOffsets[i + 1] - fileOffsets[i], &flacInfos[i], &flacFrames[i]);
            why = flacInfos[i].reason;
            infos[i] = flacAsWav(flacInfos[i]);
            sources[i] = FlacSource{ &flacInfos[i], &flacFrames[i] };
        }
        else
        {
            st = wavParse(bytes[i], fileOffsets[i + 1] - fileOffsets[i], &infos[i]);
            why = infos[i].reason;
        }
        if (st == DCS_OK && !wavLengthOk(infos[i], nullptr, why))
            st = DCS_ERR_INVALID_ARG;
        if (st != DCS_OK)
        {
            dcsCtxSetError(ctx, ("file " + std::to_string(i) + ": " + why).c_str());
            return st;
        }
    }
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        outOffsets[i + 1] = outOffsets[i] + rsMonoLength(infos[i].nValues, infos[i].channels);
    if (nFiles == 0)
        return DCS_OK;
    CacheArena held(ctx);
    std::vector<WavFile> wf;
    std::vector<uint32_t> bad;
    float *dMono = nullptr;
    ENCTRY(wavStageOnDevice(ctx, bytes.data(), infos.data(), flac ? sources.data() : nullptr, nFiles, wf, held, &dMono, bad));
    for (uint32_t i = 0 ; flac && i < nFiles ; ++i)
        if (bad[i])
        {
            dcsCtxSetError(ctx, ("file " + std::to_string(i) + ": " + stageWhy(bad[i])).c_str());
            return DCS_ERR_BAD_STREAM;
        }
    if (out == nullptr || outCap < outOffsets[nFiles])
        return DCS_ERR_CAPACITY;
    if (outOffsets[nFiles] != 0)
        ENCCHK(hipMemcpyAsync(out, dMono, sizeof(float) * outOffsets[nFiles], hipMemcpyDeviceToHost, held.stream()));
    ENCCHK(hipStreamSynchronize(held.stream()));
    return DCS_OK;
}

DcsStatus encodeFiles(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles,
                                      const DcsEncodeParams *params, const DcsResampleFilter *filter, uint32_t flags, uint8_t *out,
                                      size_t outCap, uint64_t *outOffsets, DcsEncodeFileInfo *info,
                                      const DcsLevel *levels, uint32_t nLevels, DcsLevelInfo *levelInfo)
{
    if (ctx == nullptr || outOffsets == nullptr)
        return DCS_ERR_INVALID_ARG;
    DcsResampleFilter f;
    std::string why;
    DcsStatus status = filesArgs(files, fileOffsets, nFiles, params, filter, flags, f, why);
    if (status != DCS_OK)
    {
        if (!why.empty())
            dcsCtxSetError(ctx, why.c_str());
        return status;
    }
    const bool level = levels != nullptr || nLevels != 0;
    if (level)
        ENCTRY(lvCheckLevels(ctx, levels, nLevels, nFiles, "file"));
    std::vector<FilePlan> plan;
    status = planFiles(files, fileOffsets, nFiles, params, f, flags, plan);
    if (status != DCS_OK)
    {
        for (const FilePlan &p : plan)
            if (p.status != DCS_OK)
            {
                dcsCtxSetError(ctx, p.why.c_str());
                break;
            }
        return status;
    }
    outOffsets[0] = 0;
    if (nFiles == 0)
        return DCS_OK;
    // (a DCSa container keeps this record: the stage is for the signal the converter hands the encoder)
    std::vector<DcsLevelInfo> fileLevel(level ? nFiles : 0, DcsLevelInfo{ 0.0f, 1.0f, 0.0f, 0, 0 });
    std::vector<uint32_t> wavIdx, dcsaIdx;
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        (plan[i].kind == DCS_FILE_WAV || plan[i].kind == DCS_FILE_FLAC ? wavIdx : dcsaIdx).push_back(i);
    const bool os93 = params->formatVersion != 0x9400;
    std::vector<uint64_t> size(nFiles, 0);
    std::vector<DcsEncodeFileInfo> fi(nFiles);
    // the WAV and FLAC group: upload, W0 / W1 and F1 / F2 / F3, walk, convolve, encode where it lies; the stream bytes come down into wavOut
    const uint32_t nW = static_cast<uint32_t>(wavIdx.size());
    std::vector<uint8_t> wavOut;
    std::vector<uint64_t> wavOffsets(static_cast<size_t>(nW) + 1, 0);
    if (nW != 0)
    {
        CacheArena held(ctx);               // (given back at the end of this block, before the DCSa group borrows its own)
        std::vector<DcsWavInfo> infos(nW);
        std::vector<const uint8_t *> bytes(nW);
        std::vector<FlacSource> sources(nW, FlacSource{ nullptr, nullptr });
        for (uint32_t k = 0 ; k < nW ; ++k)
        {
            const FilePlan &p = plan[wavIdx[k]];
            infos[k] = p.wav;
            bytes[k] = files + fileOffsets[wavIdx[k]];
            if (p.kind == DCS_FILE_FLAC)
                sources[k] = FlacSource{ &p.flac, &p.flacFrames };
        }
        std::vector<WavFile> wf;
        std::vector<uint32_t> bad;
        float *dMono = nullptr;
        ENCTRY(wavStageOnDevice(ctx, bytes.data(), infos.data(), sources.data(), nW, wf, held, &dMono, bad));
        for (uint32_t k = 0 ; k < nW ; ++k)
            if (bad[k])
            {
                dcsCtxSetError(ctx, ("file " + std::to_string(wavIdx[k]) + ": " + stageWhy(bad[k])).c_str());
                return DCS_ERR_BAD_STREAM;
            }
        std::vector<RsStream> hs(nW);
        for (uint32_t k = 0 ; k < nW ; ++k)
        {
            hs[k] = rsStreamOf(wf[k].nMono, infos[k].rate, f, flags);
            hs[k].inOff = wf[k].monoOff;
        }
        rsHostRoute(hs);
        float *dRes = nullptr;
        std::vector<uint32_t> peak;
        std::vector<uint64_t> resOffsets(static_cast<size_t>(nW) + 1);
        ENCTRY(rsWalkConvolve(ctx, hs, dMono, nullptr, f, wavIdx.data(), "file", held, &dRes, resOffsets.data(), peak));
        std::vector<DcsLevelInfo> li;
        if (level)
            lvPlan(levels, nLevels, wavIdx.data(), peak, li);
        for (uint32_t k = 0 ; k < nW ; ++k)
        {
            const std::string name = "file " + std::to_string(wavIdx[k]);
            const uint64_t m = resOffsets[k + 1] - resOffsets[k];
            if (m == 0 || (m + 239) / 240 > 65535)
            {
                dcsCtxSetError(ctx, (name + (m == 0 ? ": resamples to no samples" : ": resamples to more than 65 535 frames")).c_str());
                return DCS_ERR_INVALID_ARG;
            }
            const float b = wavBound(infos[k].sampleFormat);
            const float top = level ? li[k].peakOut : fromBitsU(peak[k]);
            if (!(top <= b))
            {
                char text[192];
                snprintf(text, sizeof(text), "%s: the signal the encoder reads peaks at |x| = %.9g, beyond %.9g (attenuate the input)",
                         name.c_str(), static_cast<double>(top), static_cast<double>(b));
                dcsCtxSetError(ctx, text);
                return DCS_ERR_BAD_STREAM;
            }
        }
        uint64_t cap = 0;
        std::vector<float> bound(nW);
        for (uint32_t k = 0 ; k < nW ; ++k)
            bound[k] = wavBound(infos[k].sampleFormat);
        for (uint32_t k = 0 ; k < nW ; ++k)
            cap += (os93 ? dcs_encode93_bound : dcs_encode_bound)(resOffsets[k + 1] - resOffsets[k]);
        wavOut.resize(cap ? cap : 1);
        std::vector<DcsEncodeInfo> enc(nW);
        EncInput in;
        in.sampleOffsets = resOffsets.data();
        in.nStreams = nW;
        in.devFloat = dRes;
        in.label = wavIdx.data();
        in.bound = bound.data();
        unsigned long long *dClipped = nullptr;
        if (level)
            ENCTRY(lvScale(ctx, held, dRes, resOffsets.data(), levels, nLevels, wavIdx.data(), li, &dClipped));
        status = encodeStreams(ctx, in, params, os93, EncOutput{ wavOut.data(), cap, wavOffsets.data(), enc.data(), nullptr });
        if (status != DCS_OK)
        {
            renameError(ctx, nullptr);           // (the encoder's messages give the file's own index: in.label)
            return status;
        }
        if (level)
        {
            ENCTRY(lvCollect(ctx, dClipped, li));
            for (uint32_t k = 0 ; k < nW ; ++k)
                fileLevel[wavIdx[k]] = li[k];
        }
        for (uint32_t k = 0 ; k < nW ; ++k)
        {
            DcsEncodeFileInfo &t = fi[wavIdx[k]];
            t.kind = plan[wavIdx[k]].kind;
            t.sourceFormat = infos[k].formatCode;
            t.rate = infos[k].rate;
            t.channels = infos[k].channels;
            t.nValues = infos[k].nValues;
            t.nSamples = resOffsets[k + 1] - resOffsets[k];
            t.walk = hs[k].passThrough ? DCS_FILE_WALK_NONE : hs[k].hostWalk ? DCS_FILE_WALK_HOST : DCS_FILE_WALK_DEVICE;
            t.enc = enc[k];
            size[wavIdx[k]] = wavOffsets[k + 1] - wavOffsets[k];
        }
    }
    // the DCSa group: EncodeDCSFile's copy or re-encode (dcs_transcode_streams)
    const uint32_t nD = static_cast<uint32_t>(dcsaIdx.size());
    std::vector<uint8_t> dOut;
    std::vector<uint64_t> dOffsets(static_cast<size_t>(nD) + 1, 0);
    if (nD != 0)
    {
        std::vector<DcsStreamRef> refs(nD);
        uint64_t cap = 0;
        for (uint32_t k = 0 ; k < nD ; ++k)
        {
            refs[k] = plan[dcsaIdx[k]].ref;
            cap += plan[dcsaIdx[k]].bound;
        }
        dOut.resize(cap ? cap : 1);
        std::vector<DcsTranscodeInfo> ti(nD);
        status = dcs_transcode_streams(ctx, refs.data(), nD, params, 0, dOut.data(), cap, dOffsets.data(), ti.data());
        if (status != DCS_OK)
        {
            renameError(ctx, &dcsaIdx);
            return status;
        }
        for (uint32_t k = 0 ; k < nD ; ++k)
        {
            DcsEncodeFileInfo &t = fi[dcsaIdx[k]];
            t.kind = ti[k].action == DCS_TRANSCODE_COPIED ? DCS_FILE_DCSA_COPY : DCS_FILE_DCSA_REENCODE;
            t.sourceFormat = refs[k].os;
            t.rate = 31250;
            t.channels = 1;
            t.nValues = refs[k].len;
            t.nSamples = static_cast<uint64_t>(ti[k].srcFrames) * DCS_FRAME_SAMPLES;
            t.walk = DCS_FILE_WALK_NONE;
            t.srcFrames = ti[k].srcFrames;
            t.enc = ti[k].enc;
            size[dcsaIdx[k]] = dOffsets[k + 1] - dOffsets[k];
        }
    }
    for (uint32_t i = 0 ; i < nFiles ; ++i)
        outOffsets[i + 1] = outOffsets[i] + size[i];
    if (info != nullptr)
        memcpy(info, fi.data(), sizeof(DcsEncodeFileInfo) * nFiles);
    if (level && levelInfo != nullptr)
        memcpy(levelInfo, fileLevel.data(), sizeof(DcsLevelInfo) * nFiles);
    if (out == nullptr || outCap < outOffsets[nFiles])
        return DCS_ERR_CAPACITY;
    for (uint32_t k = 0 ; k < nW ; ++k)
        memcpy(out + outOffsets[wavIdx[k]], wavOut.data() + wavOffsets[k], wavOffsets[k + 1] - wavOffsets[k]);
    for (uint32_t k = 0 ; k < nD ; ++k)
        memcpy(out + outOffsets[dcsaIdx[k]], dOut.data() + dOffsets[k], dOffsets[k + 1] - dOffsets[k]);
    return DCS_OK;
}

}  // namespace

// (a host allocation that fails is DCS_ERR_NO_MEMORY: no exception leaves the C interface)
extern "C" DcsStatus dcs_wav_decode(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles, float *out,
                                    size_t outCap, uint64_t *outOffsets)
{
    try
    {
        return wavDecode(ctx, files, fileOffsets, nFiles, out, outCap, outOffsets, false);
    }
    catch (const std::bad_alloc &)
    {
        return DCS_ERR_NO_MEMORY;
    }
}

extern "C" DcsStatus dcs_encode_files(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles,
                                      const DcsEncodeParams *params, const DcsResampleFilter *filter, uint32_t flags, uint8_t *out,
                                      size_t outCap, uint64_t *outOffsets, DcsEncodeFileInfo *info)
{
    return dcs_encode_files_level(ctx, files, fileOffsets, nFiles, params, filter, flags, out, outCap, outOffsets, info, nullptr, 0, nullptr);
}

extern "C" DcsStatus dcs_encode_files_level(DcsCtx *ctx, const uint8_t *files, const uint64_t *fileOffsets, uint32_t nFiles,
                                            const DcsEncodeParams *params, const DcsResampleFilter *filter, uint32_t flags, uint8_t *out,
                                            size_t outCap, uint64_t *outOffsets, DcsEncodeFileInfo *info,
                                            const DcsLevel *levels, uint32_t nLevels, DcsLevelInfo *levelInfo)
{
    try
    {
        return encodeFiles(ctx, files, fileOffsets, nFiles, params, filter, flags, out, outCap, outOffsets, info, levels, nLevels, levelInfo);
    }
    catch (const std::bad_alloc &)
    {
        return DCS_ERR_NO_MEMORY;
    }
}
