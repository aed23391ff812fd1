// dcs_wav.hip.h -- the WAV reader of dcs_encode_files: a RIFF/WAVE file held in memory, read as libnyquist's
// WavDecoder::LoadFromBuffer reads it (WavDecoder.cpp, Common.cpp ReadFile / ConvertToFloat32, Common.h ScanForChunk and the
// *_to_float32 macros).  Included at the end of dcs_encode.hip, after dcs_resample.hip.h: it shares that translation unit's
// floating-point contract (no contraction; the divisions by 32767, 2^23 and 2^31 are correctly rounded divisions).
//
//   W0 ima     wavImaKernel          one lane per (IMA ADPCM block, channel): the block's nibbles, serially, to int16 at
//                                    libnyquist's offsets in a staging buffer
//   W1 unpack  wavUnpackKernel<F>    one thread per mono sample: the raw payload (or W0's int16) converted as libnyquist
//                                    converts it, the stereo mean (L + R) / 2.0f; a non-finite value flags its file.  Its
//                                    output is the staged mono buffer the resampler's walk (R2) and convolution (R3) read.
//
// The host parses each file (wavParse, dcs_wav_parse), and only the `data` payloads go up.  What launches the kernels and
// drives the files of a call, WAV and FLAC alike, is dcs_encode_files.hip.h.
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
