#!/usr/bin/env python3
"""What one svslam_pose_graph_batch call costs: HIP events of timing family 13 around the kernel, not wall clock.

  python tools/pose_graph_timing.py              the three operating points on the device, the dense CPU path beside them
  python tools/pose_graph_timing.py --cpu-only   only the CPU context (numpy.linalg.solve on the 6N x 6N system of one trial)

Operating points: one graph of 1000 keyframes with 5 loops; 1024 such graphs in one call; 8192 graphs of 100 keyframes (2 loops).
Reads nothing outside the repository."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def graph(n, nloops, seed):
    import pose_graph_cases as pc
    rng = np.random.default_rng(seed)
    loops = []
    for k in range(nloops):
        i = int((k + 1) * (n - 1) / nloops)
        j = int(rng.integers(1, max(2, i // 3)))
        loops.append((i, j))
    return pc.make(n, seed, loops=loops, pts="one")


def dense_cpu(job, trials=1):
    """one LM trial of the reference's dense path: the 6n x 6n system of the start state through numpy.linalg.solve"""
    import ref_pose_graph as rpg
    poses = np.asarray(job["poses"]); fixed = np.asarray(job["fixed"]).astype(bool)
    ea, eb, meas = job["edges"]
    fidx = rpg.free_index(fixed); n = int((~fixed).sum())
    H = np.zeros((6 * n, 6 * n)); b = np.zeros(6 * n)
    for k in range(len(ea)):
        Ja, Jb = rpg.edge_jac_analytic(meas[k], poses[ea[k]], poses[eb[k]])
        e = rpg.edge_error(meas[k], poses[ea[k]], poses[eb[k]])
        for f, J in ((fidx[ea[k]], Ja), (fidx[eb[k]], Jb)):
            if f >= 0:
                H[6 * f:6 * f + 6, 6 * f:6 * f + 6] += J.T @ J; b[6 * f:6 * f + 6] -= J.T @ e
        fa, fb = fidx[ea[k]], fidx[eb[k]]
        if fa >= 0 and fb >= 0:
            H[6 * fa:6 * fa + 6, 6 * fb:6 * fb + 6] += Ja.T @ Jb; H[6 * fb:6 * fb + 6, 6 * fa:6 * fa + 6] += Jb.T @ Ja
    H += 1e-5 * np.abs(np.diag(H)).max() * np.eye(6 * n)
    best = 1e30
    for _ in range(trials):
        t = time.perf_counter(); np.linalg.solve(H, b); best = min(best, time.perf_counter() - t)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--iters", type=int, default=22)
    ap.add_argument("--big-jobs", type=int, default=1024)
    ap.add_argument("--small-jobs", type=int, default=8192)
    a = ap.parse_args()
    g1000 = graph(1000, 5, 1); g100 = graph(100, 2, 2)
    out = {"cpu_dense_solve_ms_per_trial": {"1000kf": dense_cpu(g1000, 2), "100kf": dense_cpu(g100, 5)}}
    if not a.cpu_only:
        svs = importlib.import_module("stereovision-slam_amd")
        ctx = svs.Context(64, 32, max_slots=1, max_jobs=1)
        ctx.pose_graph([g100], iters=2)                                   # warm-up: module load
        for name, jobs in (("1x1000kf_5loops", [g1000]), ("%dx1000kf_5loops" % a.big_jobs, [g1000] * a.big_jobs),
                           ("%dx100kf_2loops" % a.small_jobs, [g100] * a.small_jobs)):
            ctx.pose_graph(jobs, iters=1)                                 # scratch of this size allocated outside the measurement
            ctx.timing(True)
            t = time.perf_counter()
            res = ctx.pose_graph(jobs, iters=a.iters)
            wall = (time.perf_counter() - t) * 1e3
            ms, launches, units = ctx.timing_get("pose_graph")
            ctx.timing(False)
            out[name] = dict(device_ms=ms, wall_ms=wall, jobs=units, iters=res[0]["iters"], trials=res[0]["trials"],
                             chi2_before=res[0]["chi2_before"], chi2_after=res[0]["chi2_after"],
                             device_ms_per_trial=ms / max(res[0]["trials"], 1))
            print(name, json.dumps(out[name]), flush=True)
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
