/* Fixture generator (build container only): libsamplerate's sinc converter from the DCS rate to an output rate, between
 * libsamplerate's own int16 conversions, with the reference encoder's call pattern (DCSEncoder::WriteStream / CloseStream,
 * DCSEncoder.cpp:650-721: 16 input samples per src_process call, a 512-float output buffer, one zero-length end-of-input
 * call).
 *   out_rate_driver <in.s16> <out.s16> <out.f32> <converter 0 best | 1 medium | 2 fastest> <outRate>
 * in.s16 holds raw little-endian int16 samples at 31 250 Hz; out.f32 receives the converter's float output and out.s16
 * what src_float_to_short_array makes of it.  The ratio is (double)outRate / 31250.0 at every rate, 31 250 included. */
#include <stdio.h>
#include <stdlib.h>
#include "samplerate.h"

static float *out;
static long nOut, capOut;

static void put(const float *p, long n)
{
    if (nOut + n > capOut)
    {
        capOut = 2 * (nOut + n) + 1024;
        out = (float *)realloc(out, (size_t)capOut * sizeof(float));
    }
    for (long i = 0 ; i < n ; ++i)
        out[nOut++] = p[i];
}

static int write_stream(SRC_STATE *s, double ratio, const float *pcm, long numSamples, int eof)
{
    while (numSamples != 0 || eof)
    {
        float inbuf[16], outbuf[512];
        SRC_DATA d;
        long cur = numSamples < 16 ? numSamples : 16;
        for (long i = 0 ; i < cur ; ++i)
            inbuf[i] = *pcm++;
        numSamples -= cur;
        d.data_in = inbuf;
        d.input_frames = cur;
        d.src_ratio = ratio;
        d.end_of_input = (numSamples == 0 && eof);
        if (numSamples == 0)
            eof = 0;
        d.data_out = outbuf;
        d.output_frames = 512;
        d.output_frames_gen = 0;
        d.input_frames_used = 0;
        if (src_process(s, &d) != 0)
            return 1;
        put(outbuf, d.output_frames_gen);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: out_rate_driver <in.s16> <out.s16> <out.f32> <converter> <outRate>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (f == NULL) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    long n = 0, cap = 4096;
    short *in = (short *)malloc((size_t)cap * sizeof(short));
    size_t got;
    while ((got = fread(in + n, sizeof(short), (size_t)(cap - n), f)) != 0)
    {
        n += (long)got;
        if (n == cap) { cap *= 2; in = (short *)realloc(in, (size_t)cap * sizeof(short)); }
    }
    fclose(f);
    const int conv = atoi(argv[4]), rate = atoi(argv[5]);
    const double ratio = (double)rate / 31250.0;
    float *x = (float *)malloc((size_t)(n + 1) * sizeof(float));
    src_short_to_float_array(in, x, (int)n);
    int err = 0;
    SRC_STATE *s = src_new(conv, 1, &err);
    if (s == NULL) { fprintf(stderr, "src_new: %d\n", err); return 3; }
    src_set_ratio(s, ratio);
    if (n != 0 && write_stream(s, ratio, x, n, 0)) return 4;
    if (write_stream(s, ratio, NULL, 0, 1)) return 4;       /* the end-of-input call */
    src_delete(s);
    short *y = (short *)malloc((size_t)(nOut + 1) * sizeof(short));
    src_float_to_short_array(out, y, (int)nOut);
    FILE *o = fopen(argv[2], "wb");
    fwrite(y, sizeof(short), (size_t)nOut, o);
    fclose(o);
    o = fopen(argv[3], "wb");
    fwrite(out, sizeof(float), (size_t)nOut, o);
    fclose(o);
    return 0;
}
