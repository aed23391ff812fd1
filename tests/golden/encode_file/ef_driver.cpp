// Fixture generator (build container only): the reference's DCSEncoder::EncodeFile on one file, linked with the vendored
// libnyquist and libsamplerate.  It also records what NyquistIO::Load makes of the file, or the text of its exception.
//   ef_driver <file> <out.stream> <out.f32> <formatVersion hex> <type> <subtype>
// stdout: "load ok <channels> <rate> <values>" or "load error <text>", then "encode ok <bytes>" or "encode error <text>"
#include <stdio.h>
#include <stdlib.h>
#include <exception>
#include <string>
#include "DCSEncoder.h"
#include "libnyquist/Decoders.h"

int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: ef_driver <file> <out.stream> <out.f32> <fv> <type> <sub>\n"); return 2; }
    {
        nqr::AudioData d;
        nqr::NyquistIO loader;
        try
        {
            loader.Load(&d, argv[1]);
            FILE *o = fopen(argv[3], "wb");
            fwrite(d.samples.data(), sizeof(float), d.samples.size(), o);
            fclose(o);
            printf("load ok %d %d %zu\n", d.channelCount, d.sampleRate, d.samples.size());
        }
        catch (std::exception &e)
        {
            printf("load error %s\n", e.what());
        }
        fflush(stdout);
    }
    DCSEncoder enc;
    enc.compressionParams.formatVersion = static_cast<uint16_t>(strtoul(argv[4], nullptr, 16));
    enc.compressionParams.streamFormatType = atoi(argv[5]);
    enc.compressionParams.streamFormatSubType = atoi(argv[6]);
    DCSEncoder::DCSAudio obj;
    std::string err;
    DCSEncoder::OpenStreamStatus status;
    if (enc.EncodeFile(argv[1], obj, err, &status))
    {
        FILE *o = fopen(argv[2], "wb");
        fwrite(obj.data.get(), 1, obj.nBytes, o);
        fclose(o);
        printf("encode ok %zu\n", obj.nBytes);
    }
    else
        printf("encode error %s\n", err.c_str());
    return 0;
}
