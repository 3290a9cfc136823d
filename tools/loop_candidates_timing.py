#!/usr/bin/env python3
"""What one svslam_loop_candidates_batch call costs: HIP events of timing family 16 around the kernel, and the wall time of
the call with its upload of the queries and download of the results.

  python tools/loop_candidates_timing.py [--out profiles/loop_candidates_timing.txt]

Operating points: 1, 1024 and 8192 jobs (one per stream) of dim 1280 against stores of 4096, 768 and 96 rows per stream (21 MB, 4.0 GB,
4.0 GB: the whole store stays far under 16 GB and, for the two batched points, far above the chip's caches), min_gap 0 so that every
row is compared.  The rows are one random block appended over and over under ascending ids: the kernel's time does not depend on the
values.  bytes/s = rows compared x the 5120 bytes a padded row of dim 1280 occupies, over the device time; the fraction is of the 8.0
TB/s HBM3E specification of the MI355X (a float4 copy kernel measures 6.29 TB/s, 79 % of it).  One run each after one warm-up call of
the same shape: single, unrepeated measurements.  Reads nothing outside the repository."""
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

DIM = 1280
HBM_SPEC = 8.0e12
POINTS = {1: 4096, 1024: 768, 8192: 96}         # jobs: rows per stream


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, nargs="*", default=[1, 1024, 8192])
    a = ap.parse_args()
    svs = importlib.import_module("stereovision-slam_amd")
    rng = np.random.default_rng(16)
    lines = []
    for n in a.jobs:
        rows = POINTS.get(n, 96)
        ctx = svs.Context(64, 48, max_slots=1, max_jobs=1)
        ctx.loopdb_configure(n, rows, DIM)
        per_call = max(1, min(rows, 8192 // n))                               # rows per stream and append call: 8192 vectors a call
        block = rng.standard_normal((n * per_call, DIM)).astype(np.float32)
        streams = np.repeat(np.arange(n, dtype=np.int32), per_call)
        for r0 in range(0, rows, per_call):
            k = min(per_call, rows - r0)
            sel = (np.arange(n * per_call) % per_call) < k
            ctx.loopdb_append(streams[sel], (r0 + np.tile(np.arange(per_call), n))[sel], block[sel])
        q = rng.standard_normal((n, DIM)).astype(np.float32)
        jobs = [(s, rows) for s in range(n)]
        ctx.loop_candidates(jobs, q, min_gap=0)                               # warm-up: module load, staging of this size
        ctx.timing(True)
        t = time.perf_counter()
        res = ctx.loop_candidates(jobs, q, min_gap=0)
        wall = (time.perf_counter() - t) * 1e3
        ms, launches, units = ctx.timing_get("loop_candidates")
        ctx.timing(False)
        ctx.close()
        padded = (DIM + 255) // 256 * 256 * 4
        bps = units * padded / (ms * 1e-3)
        rec = dict(device_ms=ms, wall_ms=wall, rows_compared=units, launches=launches, store_bytes=n * rows * padded, bytes_per_s=bps,
                   fraction_of_hbm_spec=bps / HBM_SPEC, ns_per_row=1e6 * ms / max(units, 1), found=int(sum(r["status"] == 0 for r in res)))
        lines.append("%d jobs x %d rows x dim %d %s" % (n, rows, DIM, json.dumps(rec)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# single, unrepeated measurements (tools/loop_candidates_timing.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
