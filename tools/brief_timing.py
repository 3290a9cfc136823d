#!/usr/bin/env python3
"""What one svslam_brief_describe_batch call costs: HIP events of timing family 15 around the two kernels, not wall clock.

  python tools/brief_timing.py [--out profiles/brief_timing.txt]

Operating points: 1, 1024 and 8192 jobs of 150 points on 620 x 188 images (4 slots of random texture, the jobs dealt over them), the
default table, -1 degree, edge 31.  One run each: single, unrepeated measurements.  Reads nothing outside the repository."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, nargs="*", default=[1, 1024, 8192])
    a = ap.parse_args()
    svs = importlib.import_module("stereovision-slam_amd")
    w, h, nslots, npts = 620, 188, 4, 150
    rng = np.random.default_rng(15)
    ctx = svs.Context(w, h, max_slots=nslots, max_jobs=nslots)
    ctx.pyramid(list(range(nslots)), [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(nslots)])
    base = np.stack([rng.uniform(25, w - 25, (16, npts)), rng.uniform(25, h - 25, (16, npts))], axis=2).astype(np.float32)
    ctx.brief_describe([(0, base[0])])                                     # warm-up: module load
    lines = []
    for n in a.jobs:
        xy = np.ascontiguousarray(np.concatenate([base[i % 16] for i in range(n)]))
        jobs = [(i % nslots, i * npts, npts) for i in range(n)]
        ctx.brief_describe(jobs, xy)                                       # the buffer of this size allocated outside the measurement
        ctx.timing(True)
        t = time.perf_counter()
        res = ctx.brief_describe(jobs, xy)
        wall = (time.perf_counter() - t) * 1e3
        ms, launches, units = ctx.timing_get("brief")
        ctx.timing(False)
        rec = dict(device_ms=ms, wall_ms=wall, points=units, launches=launches, ns_per_point=1e6 * ms / max(units, 1),
                   described=int(sum(r[2] for r in res)))
        lines.append("%dx%d %s" % (n, npts, json.dumps(rec)))
        print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
