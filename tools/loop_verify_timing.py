#!/usr/bin/env python3
"""What one svslam_loop_verify_batch call costs: HIP events of timing family 14 around the kernel, not wall clock.

  python tools/loop_verify_timing.py [--out profiles/loop_verify_timing.txt]

Operating points: 1, 1024 and 8192 jobs of 150 x 150 descriptors (100 planted matches, a fifth of them wrong, 100 hypotheses), 16
different jobs repeated.  One run each: single, unrepeated measurements.  Reads nothing outside the repository."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, nargs="*", default=[1, 1024, 8192])
    a = ap.parse_args()
    import loop_verify_cases as lc
    svs = importlib.import_module("stereovision-slam_amd")
    base = [lc.build(seed=500 + i, nc=150, nq=150, n_match=100, wrong=0.2) for i in range(16)]
    ctx = svs.Context(64, 32, max_slots=1, max_jobs=1)
    ctx.loop_verify(base[:1], lc.CAM, lc.EXT_L)                            # warm-up: module load
    lines = []
    for n in a.jobs:
        jobs = [base[i % 16] for i in range(n)]
        ctx.loop_verify(jobs, lc.CAM, lc.EXT_L, ransac_iters=1)           # the buffer of this size allocated outside the measurement
        ctx.timing(True)
        t = time.perf_counter()
        res = ctx.loop_verify(jobs, lc.CAM, lc.EXT_L)
        wall = (time.perf_counter() - t) * 1e3
        ms, launches, units = ctx.timing_get("loop_verify")
        ctx.timing(False)
        rec = dict(device_ms=ms, wall_ms=wall, jobs=units, launches=launches, us_per_job=1e3 * ms / max(units, 1),
                   accepted=sum(r["status"] == 0 for r in res), n_matches=res[0]["n_matches"], n_inliers=res[0]["n_inliers"])
        lines.append("%dx150x150 %s" % (n, json.dumps(rec)))
        print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
