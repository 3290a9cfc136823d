#!/usr/bin/env python3
"""What one svslam_gdesc_describe_batch call costs: HIP events of timing family 17 around all kernels of the call, and the
wall time of the call with its upload of the slots and download of the vectors.

  python tools/global_desc_timing.py [--out profiles/global_desc_timing.txt] [--jobs 1 64 1024]

Operating points: 1, 64 and 1024 jobs of the full MobileNetV2 table (gdesc.mobilenet_v2_layers(), seeded random parameters: the kernels'
time does not depend on the values) at 224 x 224 on KITTI-sized slots (1241 x 376), the jobs cycling over 8 slots.  FLOP/s = 2 x the
network's multiply-adds per job x jobs over the device time; the fraction is of the 157.3 TFLOP/s f32 matrix (= vector) peak of the
MI355X.  One run each after one warm-up call of the same shape: single, unrepeated measurements.  Under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/global_desc_timing.py --jobs 64) the per-kernel rows are the k_gd_* names of
FAMILY_KERNELS["global_desc"].  Reads nothing outside the repository."""
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

F32_PEAK = 157.3e12
W, H, NSLOTS = 1241, 376, 8


def macs(layers, out_w=224, out_h=224):
    h, w, total = out_h, out_w, 0
    for op, cin, cout, stride, _, _ in layers:
        if op in (0, 1):
            h, w = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
        if op == 3:
            break
        total += {0: 9 * cin, 1: 9, 2: cin}[op] * cout * h * w
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, nargs="*", default=[1, 64, 1024])
    a = ap.parse_args()
    svs = importlib.import_module("stereovision-slam_amd")
    gd = importlib.import_module("stereovision-slam_amd.gdesc")
    layers = gd.mobilenet_v2_layers()
    prm = gd.random_params(layers, 2024)
    per_job = macs(layers)
    rng = np.random.default_rng(17)
    ctx = svs.Context(W, H, max_slots=NSLOTS, max_jobs=NSLOTS)
    ctx.pyramid(list(range(NSLOTS)), [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(NSLOTS)])
    ctx.gdesc_configure(layers, prm)
    lines = []
    for n in a.jobs:
        slots = np.arange(n, dtype=np.int32) % NSLOTS
        ctx.gdesc_describe(slots)                                           # warm-up: module load, workspace of this size
        ctx.timing(True)
        t = time.perf_counter()
        v = ctx.gdesc_describe(slots)
        wall = (time.perf_counter() - t) * 1e3
        ms, launches, units = ctx.timing_get("global_desc")
        ctx.timing(False)
        assert units == n and launches == 1 and np.isfinite(v).all()
        rec = dict(device_ms=ms, wall_ms=wall, jobs=n, launches=launches, keyframes_per_s=n / (ms * 1e-3), ms_per_job=ms / n,
                   gmac_per_job=per_job * 1e-9, tflops=2.0 * per_job * n / (ms * 1e-3) * 1e-12,
                   of_f32_matrix_peak=2.0 * per_job * n / (ms * 1e-3) / F32_PEAK)
        lines.append("%dx mobilenet_v2 224x224 %s" % (n, json.dumps(rec)))
        print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
