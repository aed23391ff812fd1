// flacref_driver.cpp -- the vendored libnyquist / libFLAC as a checker for the FLAC reader and writer (test infrastructure; built
// by `make -C oracle flacref` into oracle/_ref/dcs_flacref and, with host sanitizer flags, dcs_flacref_san).
//
//   dcs_flacref load <pack> <out> <scratch dir>
//       pack: u32 count, then per file u64 bytes and the file.  Every file is written as <scratch dir>/case.flac (NyquistIO picks
//       its decoder by the extension) and loaded with NyquistIO::Load in a CHILD PROCESS of its own: the reference overruns its
//       buffer on some files, and a crash on one file must not lose the others.  out: per file
//           i32 kind (0 loaded, 1 threw, 2 crashed), i32 channels or wait status, i32 rate, u64 n, u64 m,
//           n float32 (loaded) or n bytes of the exception's text (threw), then m bytes of what the child wrote to stderr
//       (a sanitizer's reports in the _san build).  tests/flac_fuzz_cases.py hashes the floats.
//   dcs_flacref md5 <pack>
//       FLAC__stream_decoder with MD5 checking over (file, source PCM) pairs: flac_write/fw_driver.c's main, linked in unchanged.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <unistd.h>
#include <exception>
#include <string>
#include <vector>
#include "libnyquist/Decoders.h"

extern "C" int fw_main(int argc, char **argv);

namespace {

struct Head
{
    int32_t kind, a, rate;
    uint64_t n, m;
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

// the child: Load, then the record into the pipe
int loadOne(const std::string &path, int fd)
{
    Head h{};
    nqr::AudioData d;
    nqr::NyquistIO loader;
    try
    {
        loader.Load(&d, path);
        h.kind = 0;
        h.a = d.channelCount;
        h.rate = d.sampleRate;
        h.n = d.samples.size();
        if (!writeAll(fd, &h, sizeof(h)) || !writeAll(fd, d.samples.data(), sizeof(float) * d.samples.size()))
            return 3;
    }
    catch (std::exception &e)
    {
        const std::string text = e.what();
        h.kind = 1;
        h.n = text.size();
        if (!writeAll(fd, &h, sizeof(h)) || !writeAll(fd, text.data(), text.size()))
            return 3;
    }
    return 0;
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

int loadPack(const char *packPath, const char *outPath, const std::string &dir)
{
    FILE *pack = fopen(packPath, "rb"), *out = fopen(outPath, "wb");
    uint32_t count = 0;
    if (pack == nullptr || out == nullptr || fread(&count, 4, 1, pack) != 1)
        return 2;
    const std::string flac = dir + "/case.flac", errPath = dir + "/case.stderr";
    for (uint32_t i = 0 ; i < count ; ++i)
    {
        uint64_t len;
        if (fread(&len, 8, 1, pack) != 1)
            return 2;
        std::vector<uint8_t> data(len);
        if (len != 0 && fread(data.data(), 1, len, pack) != len)
            return 2;
        FILE *c = fopen(flac.c_str(), "wb");
        if (c == nullptr || fwrite(data.data(), 1, len, c) != len || fclose(c) != 0)
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
            const int rc = loadOne(flac, fds[1]);
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
        if (WIFEXITED(status) && WEXITSTATUS(status) == 0 && got.size() >= sizeof(Head))
        {
            memcpy(&h, got.data(), sizeof(Head));
            whole = got.size() == sizeof(Head) + (h.kind == 0 ? sizeof(float) * h.n : h.n);
        }
        if (!whole)
        {
            h = Head{};
            h.kind = 2;
            h.a = status;
            got.resize(sizeof(Head));
        }
        h.m = err.size();
        fwrite(&h, sizeof(h), 1, out);
        fwrite(got.data() + sizeof(Head), 1, got.size() - sizeof(Head), out);
        fwrite(err.data(), 1, err.size(), out);
    }
    fclose(pack);
    return fclose(out) == 0 ? 0 : 2;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 5 && strcmp(argv[1], "load") == 0)
        return loadPack(argv[2], argv[3], argv[4]);
    if (argc == 3 && strcmp(argv[1], "md5") == 0)
        return fw_main(argc - 1, argv + 1);
    fprintf(stderr, "usage: dcs_flacref load <pack> <out> <scratch dir> | dcs_flacref md5 <pack>\n");
    return 2;
}
