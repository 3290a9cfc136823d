#!/usr/bin/env python
"""What one svslam_local_fusion_batch call costs: HIP events of timing family 19 around the kernel, not wall clock.

  python tools/local_fusion_timing.py [--nkf 10] [--npt 771] [--reps 30] [--windows 7]

1, 256 and 4096 jobs per call at a window of nkf keyframes and npt active landmarks (771: what the there-and-back drive of
tests/test_gpu_local_fusion_pipeline.py has when its loop closes).  Per operating point: a warm-up call, then `windows` timed
windows of `reps` calls; the figure is the median window's time per call.  Needs a device: without one it fails."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nkf", type=int, default=10); ap.add_argument("--npt", type=int, default=771)
    ap.add_argument("--reps", type=int, default=30); ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    svs = importlib.import_module("stereovision-slam_amd")
    import local_fusion_cases as lc
    ctx = svs.Context(64, 32, max_slots=1, max_jobs=2)
    base = [lc.make_job(100 + i, a.nkf, a.npt, cur_in=True, last_in=True, max_obs=6, p_bad=0.1) for i in range(8)]
    print("# svslam_local_fusion_batch, k_local_fusion: %d keyframes, %d landmarks per job; median of %d windows of %d calls (HIP events)" %
          (a.nkf, a.npt, a.windows, a.reps))
    for njobs in (1, 256, 4096):
        jobs = [base[i % 8] for i in range(njobs)]
        ctx.local_fusion(jobs)                                         # warm-up: module load, the call's buffer at this size
        per = []
        for _ in range(a.windows):
            ctx.timing(True)
            for _ in range(a.reps):
                ctx.local_fusion(jobs)
            ms, launches, units = ctx.timing_get("local_fusion")
            ctx.timing(False)
            assert launches == a.reps and units == a.reps * njobs
            per.append(1e3 * ms / a.reps)
        per.sort()
        print("jobs %5d: %9.1f us per call (windows %.1f .. %.1f), %.3f us per job" % (njobs, per[len(per) // 2], per[0], per[-1], per[len(per) // 2] / njobs), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
