"""Inputs shared by the cloud-filter tests (CPU restatement, host emulation, GPU): small clouds at which the nearest-neighbour
search and the voxel grid can go wrong.  Everything is generated; nothing is read from disk."""
import numpy as np

import ref_stereo_bm as rbm

CAM = (718.856 * 0.5, 718.856 * 0.5, 607.1928 * 0.5, 185.2157 * 0.5)
BASELINE = 0.537166
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
POSE = np.array([0.01, -0.02, 0.005, 1.0, 0.3, -0.1, 2.0])
POSE[:4] /= np.linalg.norm(POSE[:4])


def depth_crop(svs, w, h, seed=1):
    """a w x h crop of a synthetic 620 x 188 pair (centre)"""
    left, right = svs.synth_pair(seed, 0, w=620, h=188)
    y0, x0 = (188 - h) // 2, (620 - w) // 2
    return np.ascontiguousarray(left[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(right[y0:y0 + h, x0:x0 + w])


def depth_cloud_cpu(svs, w, h):
    """the restated matcher and back-projection on such a crop: (xyz f32 [n, 3], grey u8 [n]); x outer, y inner"""
    left, right = depth_crop(svs, w, h)
    xyz, pix = rbm.dense_cloud(rbm.stereo_bm(left, right), CAM, IDENT, BASELINE, POSE)
    return xyz, left.reshape(-1)[pix]


def contrast_cloud():
    """two clusters whose densities differ by 10^4 and 20 isolated far points: the far points' 50 neighbours are a cluster away"""
    rng = np.random.default_rng(5)
    a = rng.random((2000, 3)) * 0.01 + [1.0, 2.0, 3.0]                     # 2000 points in 1e-6 m^3
    b = rng.random((2000, 3)) * 0.01 ** (1.0 / 3.0) + [1.5, 2.0, 3.0]      # 2000 points in 1e-2 m^3
    far = rng.normal(size=(20, 3))
    far = far / np.linalg.norm(far, axis=1)[:, None] * rng.uniform(40.0, 90.0, (20, 1))
    return np.concatenate([a, far[:10], b, far[10:]]).astype(np.float32)


def sor_cases(svs, depth=True):
    rng = np.random.default_rng(11)
    c = {}
    for n in (0, 1, 50, 51, 52, 63, 64, 65, 1000):
        c["n%d" % n] = (rng.normal(size=(n, 3)) * [3.0, 1.0, 0.2] + [10.0, -4.0, 1.0]).astype(np.float32)
    c["coincident"] = np.tile(np.array([[1.25, -2.5, 7.0]], np.float32), (200, 1))
    p = rng.random((1500, 3)) * [4.0, 2.0, 0.0] + [0.0, 0.0, 3.5]
    c["plane"] = p.astype(np.float32)
    t = rng.random(800)
    c["line"] = np.stack([1.0 + 5.0 * t, np.full(800, 2.0), np.full(800, -1.0)], 1).astype(np.float32)
    c["duplicates"] = np.repeat((rng.random((40, 3)) * 2.0).astype(np.float32), 30, axis=0)         # 40 sites x 30 copies: ties
    c["contrast"] = contrast_cloud()
    if depth:
        c["depth"] = depth_cloud_cpu(svs, 200, 60)[0]
    return c


def voxel_cases():
    rng = np.random.default_rng(17)
    c = {}
    xyz = (rng.normal(size=(3000, 3)) * [2.0, 1.0, 0.5]).astype(np.float32)          # both signs on every axis
    rgb = rng.integers(0, 256, (3000, 3), dtype=np.uint8)
    c["negative-0.02"] = (xyz, rgb, 0.02)
    c["negative-0.5"] = (xyz, rgb, 0.5)
    one = (rng.random((100, 3)) * 0.015 + [0.021, 0.041, -0.039]).astype(np.float32)   # all inside one 2 cm voxel
    c["single-voxel"] = (one, rng.integers(0, 256, (100, 3), dtype=np.uint8), 0.02)
    c["one-point"] = (np.array([[0.5, -0.5, 2.0]], np.float32), np.array([[7, 8, 9]], np.uint8), 0.02)
    return c
