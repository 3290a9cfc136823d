"""An independent reading of the global image descriptor's contract (include/svslam.h, svslam_gdesc_*).

prep is integer numpy written from the contract's text and is meant to agree with the library in every byte.  The layers go through
torch.nn.functional.conv2d in float64 (or float32, for the size of an f32 evaluation's own error): another summation order, no claim to
bit equality; the tests hold the library to a derived rounding bound around it."""
import numpy as np
import torch
import torch.nn.functional as F

CONV3, DW3, PW, AVGPOOL = range(4)
TAPS = np.array([8, 28, 56, 72, 56, 28, 8], np.int64)          # (2, 7, 14, 18, 14, 7, 2) / 64 as /256


def blur(img):
    """cv::GaussianBlur(7 x 7, sigma 0) on 8 bits as the contract reads it: reflect-101, full horizontal sums, one rounding"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    assert h >= 4 and w >= 4
    p = np.pad(img.astype(np.int64), 3, mode="reflect")
    hs = sum(TAPS[k] * p[:, k:k + w] for k in range(7))
    v = sum(TAPS[k] * hs[k:k + h, :] for k in range(7))
    return ((v + 32768) >> 16).astype(np.uint8)


def axis(src, dst):
    """first tap, second tap, c0, c1 of every destination index"""
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * (float(src) / float(dst)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    s = np.where(lo, 0, np.where(hi, src - 1, s))
    f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, src - 1), c0, c1


def resize(img, out_w, out_h):
    img = np.asarray(img, np.uint8).astype(np.int64)
    h, w = img.shape
    xs, xs1, a0, a1 = axis(w, out_w)
    ys, ys1, b0, b1 = axis(h, out_h)
    S = img[:, xs] * a0[None, :] + img[:, xs1] * a1[None, :]              # [h, out_w]
    S0, S1 = S[ys] >> 4, S[ys1] >> 4
    out = (((b0[:, None] * S0) >> 16) + ((b1[:, None] * S1) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def prep(img, out_w=224, out_h=224, mean=(0.485, 0.456, 0.406), scale=1.0 / 255.0):
    """(resized u8 [out_h, out_w], blob f32 [3, out_h, out_w])"""
    u8 = resize(blur(img), out_w, out_h)
    pix = u8.astype(np.float32)
    sc = np.float32(scale)
    blob = np.stack([((pix - np.float32(m)).astype(np.float32) * sc).astype(np.float32) for m in mean])
    return u8, blob


def weight_shape(l):
    return {CONV3: (l[2], l[1], 3, 3), DW3: (l[2], 1, 3, 3), PW: (l[2], l[1], 1, 1)}.get(l[0])


def split(layers, params):
    params = np.asarray(params, np.float32).reshape(-1)
    out, o = [], 0
    for l in layers:
        shp = weight_shape(l)
        if shp is None:
            out.append(None)
            continue
        n = int(np.prod(shp))
        out.append((params[o:o + n].reshape(shp), params[o + n:o + n + l[2]]))
        o += n + l[2]
    assert o == params.size
    return out


def layer(l, wb, x, outs, dtype=torch.float64, absolute=False):
    """one layer on x [n, c, h, w] (torch, dtype); outs: the earlier layers' outputs.  absolute: |bias| + sum |w x| (+ |residual|)
    in place of the value, before the ReLU6: the magnitude the rounding bound multiplies"""
    op, cin, cout, stride, relu6, add_from = l
    if op == AVGPOOL:
        xx = x.abs() if absolute else x
        return xx.reshape(x.shape[0], x.shape[1], -1).sum(2) / (1.0 if absolute else float(x.shape[2] * x.shape[3]))
    w, b = (torch.from_numpy(np.ascontiguousarray(a)).to(dtype) for a in wb)
    if absolute:
        w, b, x = w.abs(), b.abs(), x.abs()
    if op == CONV3:
        y = F.conv2d(x, w, b, stride=stride, padding=1)
    elif op == DW3:
        y = F.conv2d(x, w, b, stride=stride, padding=1, groups=cin)
    else:
        y = F.conv2d(x, w, b)
    if add_from >= 0:
        y = y + (outs[add_from].abs() if absolute else outs[add_from])
    if relu6 and not absolute:
        y = y.clamp(0.0, 6.0)
    return y


def forward(layers, params, blob, dtype=torch.float64):
    """blob [n, 3, h, w] f32 -> (descriptors [n, dim] numpy of dtype, every layer's output)"""
    x = torch.from_numpy(np.ascontiguousarray(blob)).to(dtype)
    outs = []
    with torch.no_grad():
        for l, wb in zip(layers, split(layers, params)):
            x = layer(l, wb, x, outs, dtype)
            outs.append(x)
    return x.numpy(), outs


def gamma(n):
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def chain_length(l, hw_in=None):
    op = l[0]
    n = {CONV3: 9 * l[1] + 1, DW3: 10, PW: l[1] + 1}.get(op, hw_in)
    return n + (1 if l[5] >= 0 else 0)
