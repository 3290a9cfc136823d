"""Colour input of the dense program, stated in numpy: the yardstick of csrc/k_colour.h (svslam_pyramid_bgr_batch,
svslam_dense_cloud_bgr_batch) and of facade::imread(path, IMREAD_COLOR).

  grey      cv::cvtColor(COLOR_BGR2GRAY) as this project states it: (R 4899 + G 9617 + B 1868 + 8192) >> 14 in integers, the weights
            facade::read_png has always used (SVSLAM_GREY_FROM_RGB of include/svslam.h).  Parity with OpenCV's own 8-bit
            conversion is unpinned.
  size      the working size of a source: the source's own, or cvRound(src / 2) — round half to even — per axis
            (svslam_pyramid_decimate_batch's rule, src/dataset.cpp:162-165)
  decimate  cv::resize(0.5, 0.5, INTER_NEAREST): dst(x, y) = src(2x, 2y)
Conversion and decimation are both per pixel: their order does not matter."""
import numpy as np

WR, WG, WB = 4899, 9617, 1868


def grey_from_bgr(img):
    """uint8 [..., 3] (b, g, r) -> uint8 [...]"""
    a = np.asarray(img).astype(np.int64)
    return ((a[..., 2] * WR + a[..., 1] * WG + a[..., 0] * WB + 8192) >> 14).astype(np.uint8)


def cv_round_half(n):
    """cvRound(n * 0.5): round half to even"""
    return int(np.rint(n * 0.5))


def halves_to(src_w, src_h):
    return cv_round_half(src_w), cv_round_half(src_h)


def decimate(img, w, h):
    """dst(x, y) = src(2x, 2y) for x < w, y < h"""
    d = np.asarray(img)[::2, ::2]
    assert d.shape[0] >= h and d.shape[1] >= w
    return np.ascontiguousarray(d[:h, :w])


def prepare(bgr, w, h):
    """a source image uint8 [src_h, src_w, 3] at a context of w x h -> (grey uint8 [h, w], plane uint8 [h, w, 3]): what
    k_bgr_prepare writes.  The source is w x h itself, or halves to it."""
    bgr = np.asarray(bgr, np.uint8)
    sh, sw = bgr.shape[:2]
    if (sw, sh) != (w, h):
        assert halves_to(sw, sh) == (w, h), ((sw, sh), (w, h))
        bgr = decimate(bgr, w, h)
    plane = np.ascontiguousarray(bgr)
    return grey_from_bgr(plane), plane
