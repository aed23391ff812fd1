#!/usr/bin/env python3
"""Kernel time of one workload's resident batch with the library DCS_HIP_LIB names (default: the tree's), one line:
HIP events around `steps` launches, the median (min max) of fifteen such windows behind 3 000 warm-up launches -- with a
handful of warm-up launches and three windows the rounds of one box lie a microsecond apart.  Run on the GPU box, one
process per figure (tools/ab_procs.sh interleaves two libraries).

    python tools/ab_kernel.py <workload> [steps]        DCS_TAG labels the line
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dcsexplorer_amd as D
from dcsexplorer_amd import workloads

wl, steps = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 200
if wl == "realistic_65536":
    workloads.register_recordings(np.load(os.path.join(ROOT, "tests", "golden", "encoder_golden.npz")))
b = workloads.build(wl)
ctx = D.Context(0)
bt = ctx.batch(b["blob"], b["srcs"], b["jobs"])
bt.run_many(3000); bt.sync()
t = sorted(bt.time(steps) for _ in range(15))
even = int(bt.even_deal) if hasattr(bt.L, "dcs_batch_even_deal") else 0
sole = int(bt.sole_source_kernel) if hasattr(bt.L, "dcs_batch_sole_source_kernel") else 0
print("%s %-16s %.3f us (%.3f %.3f) fpw %d cpw %d even %d sole %d" % (os.environ.get("DCS_TAG", "?"), wl, t[7] * 1e3, t[0] * 1e3, t[14] * 1e3,
      bt.frames_per_wave, bt.chunks_per_wave, even, sole), flush=True)
bt.close(); ctx.close()
