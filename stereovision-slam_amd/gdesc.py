"""The global image descriptor's network as data (include/svslam.h, svslam_gdesc_*): MobileNetV2's layer table, the folding
of a torchvision state dict into the flat parameter array the library takes, seeded random parameters for tests, and one file format.

A layer is (op, cin, cout, stride, relu6, add_from) with op an index into OPS.  params holds, per layer in table order, the weights
(CONV3 [cout][cin][3][3], DW3 [c][3][3], PW [cout][cin]) followed by bias[cout]; AVGPOOL has none.

The file (save / load), little-endian: b"SVGD", u32 version = 1, u32 nlayers, nlayers x 6 i32, i32 out_w, i32 out_h, 3 f32 mean,
f32 scale, i64 workspace_bytes, i64 nparams, nparams f32.
"""
import struct

import numpy as np

OPS = ("CONV3", "DW3", "PW", "AVGPOOL")
CONV3, DW3, PW, AVGPOOL = range(4)
MAGIC = b"SVGD"
VERSION = 1
PREP_DEFAULTS = dict(out_w=224, out_h=224, mean=(0.485, 0.456, 0.406), scale=1.0 / 255.0, workspace_bytes=0)
# torchvision's MobileNetV2: expansion t, channels c, repeats n, stride s of the first repeat
_MNV2 = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))


def mobilenet_v2_layers():
    """MobileNetV2 up to the global average pool: 52 convolutions + the pool (what svslam_gdesc_mobilenet_v2 returns)"""
    T = [(CONV3, 3, 32, 2, 1, -1)]
    cin = 32
    for t, c, n, s in _MNV2:
        for i in range(n):
            stride, hid, src = (s if i == 0 else 1), cin * t, len(T) - 1
            if t != 1:
                T.append((PW, cin, hid, 1, 1, -1))
            T.append((DW3, hid, hid, stride, 1, -1))
            T.append((PW, hid, c, 1, 0, src if (stride == 1 and cin == c) else -1))
            cin = c
    T.append((PW, 320, 1280, 1, 1, -1))
    T.append((AVGPOOL, 1280, 1280, 1, 0, -1))
    return T


def mobilenet_v2_names():
    """per convolution of mobilenet_v2_layers(): (conv prefix, BatchNorm prefix) in torchvision's state dict"""
    names = [("features.0.0", "features.0.1")]
    blk = 1
    for t, c, n, s in _MNV2:
        for _ in range(n):
            p = "features.%d.conv" % blk
            if t != 1:
                names += [(p + ".0.0", p + ".0.1"), (p + ".1.0", p + ".1.1"), (p + ".2", p + ".3")]
            else:
                names += [(p + ".0.0", p + ".0.1"), (p + ".1", p + ".2")]
            blk += 1
    names.append(("features.18.0", "features.18.1"))
    return names


def weight_shape(layer):
    op, cin, cout = layer[0], layer[1], layer[2]
    return {CONV3: (cout, cin, 3, 3), DW3: (cout, 1, 3, 3), PW: (cout, cin, 1, 1)}.get(op)


def param_count(layers):
    return sum(int(np.prod(weight_shape(l))) + l[2] for l in layers if l[0] != AVGPOOL)


def split_params(layers, params):
    """[(weights in torch's conv2d shape, bias)] per layer, None for the pool"""
    params = np.asarray(params, np.float32).reshape(-1)
    if params.size != param_count(layers):
        raise ValueError("%d parameters for a table of %d" % (params.size, param_count(layers)))
    out, o = [], 0
    for l in layers:
        shp = weight_shape(l)
        if shp is None:
            out.append(None)
            continue
        n = int(np.prod(shp))
        out.append((params[o:o + n].reshape(shp), params[o + n:o + n + l[2]]))
        o += n + l[2]
    return out


def fold_state_dict(sd, layers=None, names=None, eps=1e-5):
    """torchvision's features.* convolution + BatchNorm entries -> params: w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)
    (+ the convolution's own bias times that factor, if it has one), folded in float64 and rounded once to f32"""
    layers = mobilenet_v2_layers() if layers is None else layers
    names = mobilenet_v2_names() if names is None else names
    convs = [l for l in layers if l[0] != AVGPOOL]
    if len(convs) != len(names):
        raise ValueError("%d convolutions, %d names" % (len(convs), len(names)))

    def get(k):
        v = sd[k]
        return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float64)
    parts = []
    for l, (cn, bn) in zip(convs, names):
        w = get(cn + ".weight")
        if tuple(w.shape) != weight_shape(l):
            raise ValueError("%s.weight has shape %s, the table wants %s" % (cn, tuple(w.shape), weight_shape(l)))
        k = get(bn + ".weight") / np.sqrt(get(bn + ".running_var") + float(eps))
        b = get(bn + ".bias") - get(bn + ".running_mean") * k
        if cn + ".bias" in sd:
            b = b + get(cn + ".bias") * k
        parts += [(w * k[:, None, None, None]).astype(np.float32).reshape(-1), b.astype(np.float32)]
    return np.concatenate(parts)


def random_params(layers, seed):
    """seeded parameters that keep every layer's output at roughly unit scale: weights N(0, gain / fan_in) with gain 2 in front of a
    ReLU6 and 1 otherwise, biases N(0, 0.1^2)"""
    rng = np.random.default_rng(seed)
    parts = []
    for l in layers:
        shp = weight_shape(l)
        if shp is None:
            continue
        fan_in = shp[1] * shp[2] * shp[3]
        gain = 2.0 if l[4] else 1.0
        parts += [(rng.standard_normal(int(np.prod(shp))) * np.sqrt(gain / fan_in)).astype(np.float32),
                  (rng.standard_normal(l[2]) * 0.1).astype(np.float32)]
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def save(path, layers, params, prep=None):
    p = dict(PREP_DEFAULTS)
    p.update(prep or {})
    prm = np.ascontiguousarray(params, "<f4").reshape(-1)
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<II", VERSION, len(layers)))
        for l in layers:
            f.write(struct.pack("<6i", *[int(v) for v in l]))
        f.write(struct.pack("<2i3ffqq", int(p["out_w"]), int(p["out_h"]), *[float(m) for m in p["mean"]], float(p["scale"]),
                            int(p["workspace_bytes"]), prm.size))
        f.write(prm.tobytes())


def load(path):
    """(layers, params, prep) as save wrote them"""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:4] != MAGIC:
        raise ValueError("%s is not a global-descriptor file" % path)
    ver, n = struct.unpack_from("<II", raw, 4)
    if ver != VERSION:
        raise ValueError("%s has version %d, this reader knows %d" % (path, ver, VERSION))
    o = 12
    layers = [tuple(struct.unpack_from("<6i", raw, o + 24 * i)) for i in range(n)]
    o += 24 * n
    ow, oh, m0, m1, m2, sc, wsb, npar = struct.unpack_from("<2i3ffqq", raw, o)
    o += struct.calcsize("<2i3ffqq")
    if len(raw) != o + 4 * npar:
        raise ValueError("%s: %d bytes of parameters, the header says %d" % (path, len(raw) - o, 4 * npar))
    params = np.frombuffer(raw, "<f4", npar, o).astype(np.float32)
    return layers, params, dict(out_w=ow, out_h=oh, mean=(m0, m1, m2), scale=sc, workspace_bytes=wsb)
