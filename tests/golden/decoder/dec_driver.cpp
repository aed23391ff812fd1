// dec_driver.cpp -- the reference's UNMODIFIED decoder as a stand-alone checker for the GPU decoder and for oracle/dcs_oracle.c
// (test infrastructure; built by `make -C oracle decref` into oracle/_ref/dcs_decref and, with host sanitizer flags,
// dcs_decref_san).  Neither binary is ever loaded into another process: the reference indexes its tables with whatever a damaged
// stream holds, and a crash must cost one case only.
//
//   dcs_decref decode <pack> <out>
//       pack: u32 count, then per case i32 os (0 OS93a, 1 OS93b, 2 OS94, 3 OS95), i32 volume, i32 channels (1..8), i32 frames to
//       pull, and per channel i32 level, u64 bytes and the stream.  Every case is decoded in a CHILD PROCESS of its own with the
//       recipe of ref_decode (oracle/ref_driver.cpp), which is the reference's own ROM-less one: MinHost + DCSDecoderNative +
//       InitStandalone(os) + SetDefaultVolume(volume) + SoftBoot() + LoadAudioStream(channel, ROMPointer(0, bytes), level) +
//       240 x GetNextSample() per frame; then GetStreamInfo of every channel's stream.  Bytes past a stream's end read as zero, as
//       the library and the oracle define it: each stream is copied into a buffer with 64 + 1024 zero bytes per pulled frame behind
//       it (no frame of any layout is longer than 1024 bytes).
//       The child hands the PCM over before it calls GetStreamInfo, which unpacks into a buffer of 256 words where the decoder
//       has 512: a stream that crashes only there keeps its PCM.
//       out: per case
//           i32 kind (0 decoded, 1 decoded but GetStreamInfo crashed, 2 crashed), i32 IsOK() ? 0 : -2 (kind 0) or the wait status,
//           i32 channels, i32 0, u64 n, u64 m, n int16 (240 x frames; kinds 0 and 1), per channel 4 x i32 (nFrames, nBytes,
//           formatType, formatSubType) and the 16 header bytes (kind 0), then m bytes of what the child wrote to stderr (a
//           sanitizer's reports in the _san build).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <sys/wait.h>
#include <unistd.h>
#include "DCSDecoderNative.h"

namespace {

struct Head
{
    int32_t kind, status, channels, zero;
    uint64_t n, m;
};

struct Info
{
    int32_t nFrames, nBytes, formatType, formatSubType;
    uint8_t header[16];
};

struct Case
{
    int32_t os, volume, channels, frames;
    std::vector<int32_t> levels;
    std::vector<std::vector<uint8_t>> streams;
};

bool writeAll(int fd, const void *p, size_t n)
{
    const char *c = static_cast<const char *>(p);
    while (n > 0)
    {
        const ssize_t w = write(fd, c, n);
        if (w <= 0)
            return false;
        c += w;
        n -= static_cast<size_t>(w);
    }
    return true;
}

DCSDecoder::OSVersion osFromInt(int os)
{
    switch (os)
    {
    case 0: return DCSDecoder::OSVersion::OS93a;
    case 1: return DCSDecoder::OSVersion::OS93b;
    case 2: return DCSDecoder::OSVersion::OS94;
    default: return DCSDecoder::OSVersion::OS95;
    }
}

// the child: decode, then the record into the pipe
int decodeOne(const Case &c, int fd)
{
    std::vector<std::vector<uint8_t>> bufs(c.streams);
    for (auto &b : bufs)
        b.resize(b.size() + 64 + 1024 * static_cast<size_t>(c.frames), 0);
    std::vector<int16_t> pcm(240 * static_cast<size_t>(c.frames));
    std::vector<Info> infos(c.channels);
    Head h{};
    {
        DCSDecoder::MinHost host;
        DCSDecoderNative dec(&host);
        dec.InitStandalone(osFromInt(c.os));
        dec.SetDefaultVolume(c.volume);
        dec.SoftBoot();
        for (int i = 0 ; i < c.channels ; ++i)
            dec.LoadAudioStream(i, DCSDecoder::ROMPointer(0, bufs[i].data()), c.levels[i]);
        for (size_t k = 0 ; k < pcm.size() ; ++k)
            pcm[k] = dec.GetNextSample();
        h.status = dec.IsOK() ? 0 : -2;
    }
    h.kind = 0;
    h.channels = c.channels;
    h.n = pcm.size();
    if (!writeAll(fd, &h, sizeof(h)) || !writeAll(fd, pcm.data(), sizeof(int16_t) * pcm.size()))
        return 3;
    for (int i = 0 ; i < c.channels ; ++i)
    {
        DCSDecoder::MinHost host;
        DCSDecoderNative dec(&host);
        dec.InitStandalone(osFromInt(c.os));
        dec.SoftBoot();
        auto si = dec.GetStreamInfo(DCSDecoder::ROMPointer(0, bufs[i].data()));
        infos[i].nFrames = si.nFrames;
        infos[i].nBytes = si.nBytes;
        infos[i].formatType = si.formatType;
        infos[i].formatSubType = si.formatSubType;
        memcpy(infos[i].header, si.header, 16);
    }
    return writeAll(fd, infos.data(), sizeof(Info) * infos.size()) ? 0 : 3;
}

std::vector<char> slurp(const std::string &path)
{
    std::vector<char> out;
    FILE *f = fopen(path.c_str(), "rb");
    if (f == nullptr)
        return out;
    char buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0 && out.size() < (1u << 16))
        out.insert(out.end(), buf, buf + n);
    fclose(f);
    return out;
}

bool readCase(FILE *pack, Case &c)
{
    int32_t head[4];
    if (fread(head, 4, 4, pack) != 4)
        return false;
    c.os = head[0]; c.volume = head[1]; c.channels = head[2]; c.frames = head[3];
    if (c.channels < 1 || c.channels > 8 || c.frames < 0 || c.frames > 65535)
        return false;
    c.levels.assign(c.channels, 0);
    c.streams.assign(c.channels, {});
    for (int i = 0 ; i < c.channels ; ++i)
    {
        uint64_t len;
        if (fread(&c.levels[i], 4, 1, pack) != 1 || fread(&len, 8, 1, pack) != 1 || len > (1u << 26))
            return false;
        c.streams[i].resize(len);
        if (len != 0 && fread(c.streams[i].data(), 1, len, pack) != len)
            return false;
    }
    return true;
}

int decodePack(const char *packPath, const char *outPath)
{
    FILE *pack = fopen(packPath, "rb"), *out = fopen(outPath, "wb");
    uint32_t count = 0;
    if (pack == nullptr || out == nullptr || fread(&count, 4, 1, pack) != 1)
        return 2;
    const std::string errPath = std::string(outPath) + ".stderr";
    for (uint32_t i = 0 ; i < count ; ++i)
    {
        Case c;
        if (!readCase(pack, c))
            return 2;
        int fds[2];
        if (pipe(fds) != 0)
            return 2;
        fflush(out);
        const pid_t pid = fork();
        if (pid < 0)
            return 2;
        if (pid == 0)
        {
            close(fds[0]);
            if (freopen(errPath.c_str(), "w", stderr) == nullptr)
                _exit(4);
            alarm(60);                  // a case is a few dozen frames: a child that runs this long never ends
            const int rc = decodeOne(c, fds[1]);
            fflush(stderr);
            _exit(rc);
        }
        close(fds[1]);
        std::vector<char> got;
        char buf[1 << 16];
        ssize_t r;
        while ((r = read(fds[0], buf, sizeof(buf))) > 0)
            got.insert(got.end(), buf, buf + r);
        close(fds[0]);
        int status = 0;
        waitpid(pid, &status, 0);
        const std::vector<char> err = slurp(errPath);
        Head h{};
        bool whole = false;
        if (got.size() >= sizeof(Head))
        {
            memcpy(&h, got.data(), sizeof(Head));
            const size_t pcmEnd = sizeof(Head) + sizeof(int16_t) * h.n;
            whole = WIFEXITED(status) && WEXITSTATUS(status) == 0 && h.kind == 0
                && got.size() == pcmEnd + sizeof(Info) * static_cast<size_t>(h.channels);
            if (!whole && h.kind == 0 && h.channels == c.channels && h.n == 240u * static_cast<size_t>(c.frames) && got.size() >= pcmEnd
                && !(WIFEXITED(status) && WEXITSTATUS(status) == 0))
            {
                h.kind = 1;
                h.status = status;
                got.resize(pcmEnd);
                whole = true;
            }
        }
        if (!whole)
        {
            h = Head{};
            h.kind = 2;
            h.status = status;
            h.channels = c.channels;
            got.resize(sizeof(Head));
        }
        h.m = err.size();
        fwrite(&h, sizeof(h), 1, out);
        fwrite(got.data() + sizeof(Head), 1, got.size() - sizeof(Head), out);
        fwrite(err.data(), 1, err.size(), out);
    }
    fclose(pack);
    unlink(errPath.c_str());
    return fclose(out) == 0 ? 0 : 2;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 4 && strcmp(argv[1], "decode") == 0)
        return decodePack(argv[2], argv[3]);
    fprintf(stderr, "usage: dcs_decref decode <pack> <out>\n");
    return 2;
}
