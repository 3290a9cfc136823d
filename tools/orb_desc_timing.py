#!/usr/bin/env python3
"""What one svslam_orb_describe_batch call costs: HIP events of timing family 21 around a call's kernels, not wall clock.

  python tools/orb_desc_timing.py [--out profiles/orb_desc_timing.txt]

Operating points: 1, 1024 and 8192 jobs of 150 keypoints on 620 x 188 synthetic frames (4 slots, the jobs dealt over them).  Two
sets of keypoints: all at octave 0 and -1 degree (what tracked features and GFTT corners carry: no level is built), and the
detector's own (svslam_orb_detect_batch on the slot, nfeatures 150, repeated up to 150 rows: its octave mix, levels 1 .. 7 built
per job).  After a warm-up call of the same size: 5 windows of one call each, the median.  As the yardstick
svslam_brief_describe_batch on the same positions in the same process, alternated with the oriented windows.  Single measurements
of one machine; no speed is promised.  Reads nothing outside the repository."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, NSLOTS, NPTS, WINDOWS = 620, 188, 4, 150, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, nargs="*", default=[1, 1024, 8192])
    a = ap.parse_args()
    svs = importlib.import_module("stereovision-slam_amd")
    ctx = svs.Context(W, H, max_slots=NSLOTS, max_jobs=256)
    ctx.pyramid(list(range(NSLOTS)), [svs.synth_pair(1 + s, 0)[0] for s in range(NSLOTS)])
    found = ctx.orb_detect([(s, None) for s in range(NSLOTS)], max_out=2 * NPTS, nfeatures=NPTS)
    detected = [np.resize(k, NPTS) for k, _ in found]
    flat = []
    for k in detected:
        t = k.copy(); t["angle"] = -1.0; t["octave"] = 0
        flat.append(t)
    mix = np.bincount(np.concatenate(detected)["octave"], minlength=8).tolist()
    lines = ["620x188, %d keypoints per job; the detector's octave mix over %d slots: %s; median of %d windows of one call" % (NPTS, NSLOTS, mix, WINDOWS)]
    print(lines[0], flush=True)
    for n in a.jobs:
        rec = dict(jobs=n, points=n * NPTS)
        for name, sets in (("octave0", flat), ("detector_mix", detected)):
            jobs = [(i % NSLOTS, sets[i % NSLOTS]) for i in range(n)]
            bjobs = [(i % NSLOTS, np.stack([sets[i % NSLOTS]["x"], sets[i % NSLOTS]["y"]], axis=1)) for i in range(n)]
            kept = sum(k for _, _, k in ctx.orb_describe(jobs))             # warm-up: module load, the buffer of this size
            ctx.brief_describe(bjobs)
            od, br = [], []
            for _ in range(WINDOWS):
                ctx.timing(True)
                ctx.orb_describe(jobs)
                ctx.brief_describe(bjobs)
                od.append(ctx.timing_get("orb_desc")[0]); br.append(ctx.timing_get("brief")[0])
                ctx.timing(False)
            o, b = float(np.median(od)), float(np.median(br))
            rec[name] = dict(rows_kept=kept, orb_desc_ms=o, orb_desc_ns_per_point=1e6 * o / (n * NPTS), brief_ms=b, brief_ns_per_point=1e6 * b / (n * NPTS),
                             ratio=o / b, orb_desc_ms_windows=[round(v, 4) for v in od])
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
