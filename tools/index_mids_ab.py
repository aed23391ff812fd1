#!/usr/bin/env python3
"""tools/index_mids_ab.py [-r rounds] parent.so new.so   -- host only, no GPU.
Host time of the many-stream index walk with and without mid records (dcs_index_streams_mids / dcs_index_streams), two builds
of the library against each other: 4 096 streams x 64 frames of the survey3 shape (12 bands, synth profile 5), at 1 and at 16
threads.  Each build runs in a process of its own, the processes interleaved round by round (parent, new, parent, ...); inside a
process the two entries alternate and the best of three calls counts.  The entries are timed on buffers made beforehand, so
what is measured is the walk and not numpy's allocations.  Prints, per build, thread count and entry, the median over the
rounds and their spread, in us per frame."""
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
N_STREAMS, N_FRAMES, THREADS = 4096, 64, (1, 16)


def child():
    import numpy as np
    import dcsexplorer_amd as D
    from dcsexplorer_amd import api, workloads
    L = D.load_library()
    streams = workloads.streams_survey3_65536(N_STREAMS, N_FRAMES)
    keep = [np.frombuffer(s[1], dtype=np.uint8) for s in streams]
    refs = (api.StreamRef * len(streams))()
    for k, s in enumerate(streams):
        refs[k].data, refs[k].len, refs[k].os = keep[k].ctypes.data, keep[k].size, s[0]
    first = (np.arange(len(streams) + 1) * N_FRAMES).astype(np.uint64)
    out = np.zeros(int(first[-1]), dtype=api.INDEX_DTYPE)
    infos = np.zeros(len(streams), dtype=api.INFO_DTYPE)
    mids = np.zeros((out.size, 16), dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    res = {}
    for threads in THREADS:
        for _ in range(3):
            for key in ("mids", "plain"):
                args = (refs, len(streams), threads, p(out), p(first), p(infos)) + ((p(mids),) if key == "mids" else ())
                t0 = time.perf_counter()
                st = (L.dcs_index_streams_mids if key == "mids" else L.dcs_index_streams)(*args)
                us = (time.perf_counter() - t0) * 1e6 / out.size
                assert st == 0 and int(infos["nValidFrames"].sum()) == out.size
                res["%d %s" % (threads, key)] = min(us, res.get("%d %s" % (threads, key), us))
    print(json.dumps(res))


def main(argv):
    rounds = 5
    if argv[:1] == ["-r"]:
        rounds, argv = int(argv[1]), argv[2:]
    libs = dict(parent=os.path.realpath(argv[0]), new=os.path.realpath(argv[1]))
    got = {}
    for r in range(rounds):
        for tag, lib in libs.items():
            env = dict(os.environ, DCS_HIP_LIB=lib)
            line = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child"], env=env, timeout=600)
            for key, us in json.loads(line.decode().strip().splitlines()[-1]).items():
                got.setdefault((key, tag), []).append(us)
    print("us per frame, %d streams x %d frames, %d rounds: median (min .. max)" % (N_STREAMS, N_FRAMES, rounds))
    for key in sorted({k for k, _ in got}, key=lambda k: (int(k.split()[0]), k)):
        for tag in libs:
            v = got[(key, tag)]
            print("  %2s threads %-5s %-6s %.4f (%.4f .. %.4f)" % (*key.split(), tag, statistics.median(v), min(v), max(v)))


if __name__ == "__main__":
    child() if sys.argv[1:] == ["--child"] else main(sys.argv[1:])
