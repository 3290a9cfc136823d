#!/usr/bin/env python3
"""What one svslam_orb_detect_batch call costs: HIP events of timing family 20 around a call's kernels, not wall clock.

  python tools/orb_timing.py [--out profiles/orb_timing.txt]

Operating points: 1, 256 and 4096 jobs on 620 x 188 synthetic frames (4 slots, the jobs dealt over them), nfeatures 150, 100 rects
per job, ORB's defaults otherwise.  After a warm-up call of the same size: 7 windows of one call each, the median.  Reported per job:
device time, and the GB/s that time implies against the bytes the levels must at least read and write (resize of image and mask,
the level-0 mask, FAST's read of image and mask, the kept-score map written and read over the interior).  For context
svslam_gftt_batch on the same slots and rects in the same process, alternated with the ORB windows, at the sizes its context's
max_jobs (256) admits.  Reads nothing outside the repository."""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, NSLOTS, NRECT, NFEATURES, EDGE, WINDOWS, GFTT_MAX_JOBS = 620, 188, 4, 100, 150, 31, 7, 256


def min_bytes_per_job():
    f = np.float32
    sizes = [(W, H)]
    for lv in range(1, 8):
        inv = f(1.0) / f(math.pow(float(f(1.2)), float(lv)))
        sizes.append((int(np.rint(f(W) * inv)), int(np.rint(f(H) * inv))))
    total = W * H                                                   # the level-0 mask is written
    for lv, (w, h) in enumerate(sizes):
        if lv:
            total += 2 * (sizes[lv - 1][0] * sizes[lv - 1][1] + w * h)      # image and mask: read the level below, write this one
        if w > 2 * EDGE and h > 2 * EDGE:
            total += 2 * w * h + 2 * (w - 2 * EDGE) * (h - 2 * EDGE)        # FAST reads image and mask; kept scores written and read
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, nargs="*", default=[1, 256, 4096])
    a = ap.parse_args()
    svs = importlib.import_module("stereovision-slam_amd")
    rng = np.random.default_rng(20)
    ctx = svs.Context(W, H, max_slots=NSLOTS, max_jobs=GFTT_MAX_JOBS)
    ctx.pyramid(list(range(NSLOTS)), [svs.synth_pair(1 + s, 0)[0] for s in range(NSLOTS)])
    rects = [np.stack([rng.uniform(0, W, NRECT), rng.uniform(0, H, NRECT)], axis=1).astype(np.float32) for _ in range(16)]
    per_job = min_bytes_per_job()
    lines = ["620x188, nfeatures %d, %d rects per job, at least %d bytes per job; median of %d windows of one call" % (NFEATURES, NRECT, per_job, WINDOWS)]
    print(lines[0], flush=True)
    for n in a.jobs:
        jobs = [(i % NSLOTS, rects[i % 16]) for i in range(n)]
        with_gftt = n <= GFTT_MAX_JOBS
        found = ctx.orb_detect(jobs, max_out=2 * NFEATURES, nfeatures=NFEATURES)                 # warm-up: module load, the buffer of this size
        if with_gftt:
            ctx.gftt(jobs, max_corners=NFEATURES)
        orb_ms, gftt_ms = [], []
        for _ in range(WINDOWS):
            ctx.timing(True)
            ctx.orb_detect(jobs, max_out=2 * NFEATURES, nfeatures=NFEATURES)
            if with_gftt:
                ctx.gftt(jobs, max_corners=NFEATURES)
            orb_ms.append(ctx.timing_get("orb")[0])
            gftt_ms.append(ctx.timing_get("gftt")[0])
            ctx.timing(False)
        ms = float(np.median(orb_ms))
        rec = dict(jobs=n, orb_device_ms=ms, orb_us_per_job=1e3 * ms / n, orb_min_GBps=per_job * n / (ms * 1e-3) / 1e9,
                   keypoints_per_job=float(np.mean([f for _, f in found])), orb_ms_windows=[round(v, 4) for v in orb_ms])
        if with_gftt:
            g = float(np.median(gftt_ms))
            rec.update(gftt_device_ms=g, gftt_us_per_job=1e3 * g / n)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
