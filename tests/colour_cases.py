"""Inputs of the colour tests: colour stereo pairs with known disparities.

Per channel an independent texture — 0.6 x (noise box-smoothed with 3 taps) + 0.4 x (the same with 9 taps), scaled to 0 .. 255 —
on a canvas wider than the image.  The image is cut into four horizontal bands of constant disparity d, with
right(x) = left(x + d) taken from the canvas.  Independent channels make almost every pixel's b, g, r pairwise different, so a
colour taken from the wrong pixel, the wrong channel or the wrong plane shows."""
import struct
import zlib

import numpy as np

# (source size, context size, full-resolution disparities of the four bands, matcher (num_disparities, block_size))
DIRECT = ((97, 53), (97, 53), (6, 11, 17, 23), (32, 5))
DEC_DOWN = ((401, 121), (200, 60), (60, 110, 170, 220), (128, 15))       # both axes round down: last source column and row unused
DEC_UP = ((403, 123), (202, 62), (60, 110, 170, 220), (128, 15))         # both round up: the last output column and row read the last source ones
KITTI = ((1241, 376), (620, 188), (20, 40, 60, 80), (128, 15))


def _box(a, taps):
    k = np.ones(taps) / taps
    a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, a)
    return np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, a)


def texture(rng, h, w):
    n = rng.standard_normal((h + 16, w + 16))
    t = (0.6 * _box(n, 3) + 0.4 * _box(n, 9))[8:-8, 8:-8]
    t = (t - t.min()) / (t.max() - t.min())
    return np.clip(np.rint(t * 255.0), 0, 255).astype(np.uint8)


def stereo_pair(seed, size, disparities):
    """(left, right) uint8 [h, w, 3] in b, g, r"""
    w, h = size
    rng = np.random.default_rng(seed)
    canvas = np.stack([texture(rng, h, w + max(disparities)) for _ in range(3)], -1)
    left = np.ascontiguousarray(canvas[:, :w])
    right = np.zeros_like(left)
    edges = [h * i // len(disparities) for i in range(len(disparities) + 1)]
    for d, y0, y1 in zip(disparities, edges[:-1], edges[1:]):
        right[y0:y1] = canvas[y0:y1, d:d + w]
    return left, right


def strided(img, extra):
    """the same image as a view whose rows are `extra` bytes further apart than tight"""
    h, w, _ = img.shape
    buf = np.full((h, 3 * w + extra), 0xA5, np.uint8)
    buf[:, :3 * w] = img.reshape(h, 3 * w)
    return np.lib.stride_tricks.as_strided(buf, (h, w, 3), (3 * w + extra, 3, 1))


def png_filter_rows(arr, filters):
    """PNG's forward filters 0..4 on uint8 [h, w, ch]; filters[y] is the type of row y"""
    h, w, ch = arr.shape
    raw = arr.reshape(h, w * ch).astype(np.int32)
    out = bytearray()
    for y in range(h):
        ft = filters[y % len(filters)]
        cur = raw[y]
        prev = raw[y - 1] if y else np.zeros_like(cur)
        a = np.concatenate([np.zeros(ch, np.int32), cur[:-ch]])
        c = np.concatenate([np.zeros(ch, np.int32), prev[:-ch]])
        b = prev
        if ft == 0:
            pred = np.zeros_like(cur)
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = b
        elif ft == 3:
            pred = (a + b) >> 1
        else:
            p = a + b - c
            pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out.append(ft)
        out += ((cur - pred) & 0xff).astype(np.uint8).tobytes()
    return bytes(out)


def write_png(path, arr, filters=(0,)):
    """an 8-bit PNG of uint8 [h, w] or [h, w, 1..4] (grey, grey + alpha, r g b, r g b a), row y filtered with type filters[y % len]"""
    arr = np.asarray(arr, np.uint8)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    h, w, ch = arr.shape
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[ch]

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(png_filter_rows(arr, filters), 6)) + chunk(b"IEND", b""))
