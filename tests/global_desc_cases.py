"""Cases of the global image descriptor shared by the host-build and the device tests: the host build's loader and call wrappers, the
small networks whose shapes sit where the tiling can go wrong, seeded images and parameters, and the refusals with their accepted
neighbours."""
import ctypes as C
import importlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONV3, DW3, PW, AVGPOOL = range(4)
PREP_SIZES = [(4, 4), (5, 9), (97, 53), (620, 188), (1241, 376)]            # (w, h)
OUT_SIZES = [(224, 224), (13, 7)]
DEVICE_PREP_SIZES = [(97, 53), (620, 188), (1241, 376)]                     # a context is 16 x 16 at the least
NSLOTS = 3


class GdLayer(C.Structure):
    _fields_ = [("op", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("stride", C.c_int), ("relu6", C.c_int), ("add_from", C.c_int)]


class GdPrep(C.Structure):
    _fields_ = [("out_w", C.c_int), ("out_h", C.c_int), ("mean", C.c_float * 3), ("scale", C.c_float), ("workspace_bytes", C.c_longlong)]


PREP_DEFAULTS = dict(out_w=224, out_h=224, mean=(0.485, 0.456, 0.406), scale=1.0 / 255.0, workspace_bytes=0)


def gdesc():
    return importlib.import_module("stereovision-slam_amd.gdesc")


_emu = None


def load_emu():
    """csrc/k_global_desc.h compiled for the host: the package's lib/libgd_host_emu.so when the build left it, else compiled here"""
    global _emu
    if _emu is None:
        L = C.CDLL(importlib.import_module("stereovision-slam_amd.build").build_emu("gd"))
        L.emu_gd_error.restype = C.c_char_p
        L.emu_gd_job_floats.restype = C.c_longlong
        L.emu_gd_configure.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
        L.emu_gd_describe.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.emu_gd_pw_tiles.argtypes = [C.c_longlong, C.c_int, C.c_int]
        _emu = L
    return _emu


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def prep_struct(prep):
    if prep is None:
        return None
    p = dict(PREP_DEFAULTS); p.update(prep)
    return GdPrep(int(p["out_w"]), int(p["out_h"]), (C.c_float * 3)(*[float(m) for m in p["mean"]]), float(p["scale"]), int(p["workspace_bytes"]))


def emu_configure(w, h, layers, params, prep=None, nparams=None):
    """(rc, message)"""
    L = load_emu()
    arr = (GdLayer * max(len(layers), 1))(*[GdLayer(*[int(v) for v in l]) for l in layers])
    prm = np.ascontiguousarray(params, np.float32).reshape(-1)
    P = prep_struct(prep)
    rc = L.emu_gd_configure(int(w), int(h), len(layers), C.cast(arr, C.c_void_p), _p(prm), prm.size if nparams is None else int(nparams),
                            C.cast(C.pointer(P), C.c_void_p) if P is not None else None)
    return rc, (L.emu_gd_error().decode() if rc else "")


def emu_describe(imgs, slots, out_wh=None, dump=None, vecs=None):
    """imgs [nslots, h, w] u8 (the size the network was configured for).  Returns dict(rc, msg, vecs, u8, blob, dump); dump = (layer
    index, floats per job) asks for that layer's output"""
    L = load_emu()
    imgs = np.ascontiguousarray(imgs, np.uint8)
    sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
    n, dim = len(sl), L.emu_gd_dim()
    if vecs is None:
        vecs = np.zeros((n, max(dim, 1)), np.float32)
    u8 = blob = d = None
    if out_wh is not None:
        u8 = np.zeros((n, out_wh[1], out_wh[0]), np.uint8); blob = np.zeros((n, 3, out_wh[1], out_wh[0]), np.float32)
    if dump is not None:
        d = np.zeros((n, dump[1]), np.float32)
    rc = L.emu_gd_describe(len(imgs), _p(imgs), n, _p(sl), _p(vecs), _p(u8), _p(blob), dump[0] if dump else -1, _p(d))
    return dict(rc=rc, msg=L.emu_gd_error().decode() if rc else "", vecs=vecs, u8=u8, blob=blob, dump=d)


def images(w, h, seed=0, n=NSLOTS):
    """n different u8 images: smooth structure + noise + a few saturated patches, so that blur, rounding and both resize taps matter"""
    rng = np.random.default_rng(1000 * w + h + seed)
    out = []
    for k in range(n):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        im = 128 + 90 * np.sin(xx / (3.0 + k) + k) * np.cos(yy / (4.0 + k)) + rng.normal(0, 25, (h, w))
        im[: max(h // 5, 1), : max(w // 5, 1)] = 255 * (k & 1)
        out.append(np.clip(np.rint(im), 0, 255).astype(np.uint8))
    return np.stack(out)


def seeded(layers, seed):
    return gdesc().random_params(layers, seed)


# ---- the small networks -----------------------------------------------------------------------------------------------------------
def tiny_net():
    """every channel count below one tile; prep output 16 x 16"""
    return [(CONV3, 3, 5, 2, 1, -1), (DW3, 5, 5, 1, 1, -1), (PW, 5, 7, 1, 1, -1), (PW, 7, 5, 1, 0, 1), (AVGPOOL, 5, 5, 1, 0, -1)], (16, 16)


def pw_net(cin, cout, relu6=0):
    """PW 3 -> cin feeds the PW cin -> cout under test"""
    return [(PW, 3, cin, 1, 0, -1), (PW, cin, cout, 1, relu6, -1), (AVGPOOL, cout, cout, 1, 0, -1)]


def dw_net(stride):
    return [(DW3, 3, 3, stride, 0, -1), (AVGPOOL, 3, 3, 1, 0, -1)]


def conv_net(stride, cout=5):
    return [(CONV3, 3, cout, stride, 0, -1), (AVGPOOL, cout, cout, 1, 0, -1)]


PW_EDGES = (31, 32, 33, 63, 64, 65)
# name -> (layers, (out_w, out_h)): the single-layer shapes of the issue
LAYER_CASES = {}
for _s, _wh in ((2, (7, 7)), (2, (8, 8)), (1, (1, 1)), (1, (2, 2)), (2, (7, 8))):
    LAYER_CASES["dw3_s%d_%dx%d" % (_s, _wh[0], _wh[1])] = (dw_net(_s), _wh)
for _s in (1, 2):
    LAYER_CASES["conv3_s%d_5x3" % _s] = (conv_net(_s), (5, 3))
LAYER_CASES["pw_960_320_7x7"] = (pw_net(960, 320), (7, 7))
LAYER_CASES["tiny"] = tiny_net()


def case_prep(wh, **more):
    p = dict(out_w=wh[0], out_h=wh[1]); p.update(more)
    return p


# ---- the batch cases: job counts at which the launcher takes k_gd_pw_mfma<4> and <2> (tests/test_gpu_global_desc_batch.py) ----------
BATCH_WH = (7, 5)                            # 35 pixels per job: a pixel tile of 32 straddles two jobs
BATCH_HW = BATCH_WH[0] * BATCH_WH[1]
JOBS_NT4, JOBS_NT4_EXACT, JOBS_NT2 = 1873, 1872, 1871          # 2049, 2048 and 2047 pixel tiles


def pw_tiles(hw, njobs, cout):
    """the NT of k_gd_pw_mfma<NT> the launcher takes for a PW layer (csrc/k_global_desc.h, gd_pw_tiles)"""
    return int(load_emu().emu_gd_pw_tiles(int(hw), int(njobs), (int(cout) + 31) & ~31))


def batch_net(cin, cout, relu6=0):
    """PW 3 -> cin, the PW cin -> cout under test, and a DW3 in front of the pool: its 9 taps make the result depend on where each
    pixel of the PW's output landed, which the pool's sum alone often does not"""
    return [(PW, 3, cin, 1, 0, -1), (PW, cin, cout, 1, relu6, -1), (DW3, cout, cout, 1, 0, -1), (AVGPOOL, cout, cout, 1, 0, -1)]


def batch_residual_net():
    return [(PW, 3, 40, 1, 0, -1), (PW, 40, 130, 1, 1, -1), (PW, 130, 40, 1, 0, 0), (DW3, 40, 40, 1, 0, -1), (AVGPOOL, 40, 40, 1, 0, -1)]


def big_cout_net():
    """the largest cout a table may hold, on a 1 x 1 prep: k_gd_conv3's grid.y is cout"""
    return [(CONV3, 3, 1 << 16, 1, 0, -1), (PW, 1 << 16, 4, 1, 0, -1), (AVGPOOL, 4, 4, 1, 0, -1)], (1, 1)


def batch_slots(n):
    """neighbouring jobs read different images"""
    return np.asarray((2, 0, 1), np.int32)[np.arange(n) % 3]


def param_spans(layers):
    """per layer (start of the weights, start of the bias, end) in the flat parameter array"""
    out, o = [], 0
    for l in layers:
        nw = {CONV3: l[2] * l[1] * 9, DW3: l[2] * 9, PW: l[2] * l[1]}.get(l[0])
        if nw is None:
            out.append((o, o, o))
            continue
        out.append((o, o + nw, o + nw + l[2]))
        o += nw + l[2]
    return out


def scale_bias(layers, prm, f):
    prm = np.array(prm, np.float32)
    for w0, b0, e in param_spans(layers):
        prm[b0:e] *= np.float32(f)
    return prm


def zero_bias(layers, prm):
    return scale_bias(layers, prm, 0.0)


def scale_weights(layers, prm, li, f):
    prm = np.array(prm, np.float32)
    w0, b0, e = param_spans(layers)[li]
    prm[w0:b0] *= np.float32(f)
    return prm


SUBNORMAL_REGIMES = ("activations", "weights", "edge")


def subnormal_case(regime, seed=11):
    """(layers, params, prep, classes the host result has to hold): f32 subnormals as the MFMA's B input and accumulator (activations:
    the blob is (pix - mean) 2^-134), as its A input (weights: the first layer's times 2^-130), and accumulators that cross the edge of
    the normal range (edge: blob times 2^-128 against biases times 2^-118)"""
    layers = batch_net(33, 65)
    prm = seeded(layers, seed)
    if regime == "activations":
        return layers, zero_bias(layers, prm), case_prep(BATCH_WH, scale=2.0 ** -134), ("subnormal",)
    if regime == "weights":
        return layers, scale_weights(layers, zero_bias(layers, prm), 0, 2.0 ** -130), case_prep(BATCH_WH), ("subnormal",)
    assert regime == "edge"
    return layers, scale_bias(layers, prm, 2.0 ** -118), case_prep(BATCH_WH, scale=2.0 ** -128), ("subnormal", "normal")


def overflow_case(relu6, imgs, seed=13):
    """(layers, params, prep): infinities enter the PW 33 -> 65 under test and NaN arises inside its chain.  A chain of fmaf over finite
    inputs never gives NaN (a product is exact, so inf - inf needs an infinite input), hence the infinities are made one layer earlier,
    by the first PW: with mean 0 and scale = (FLT_MAX / 3e38) / (t - 0.5) its weights (3e38, 0, 0) and (-3e38, 0, 0) make channel 0
    +inf and channel 1 -inf at the pixels >= t and leave them finite elsewhere; t is one above the largest pixel of the darkest of
    imgs (the resized u8 images by ref_global_desc, which equal the library's in every byte), so one image stays finite throughout.
    Output channel co of the layer under test, by co % 8, at a pixel >= t: 0: weights (0.25, -0.25) on inputs 0 and 1, +inf; 1:
    (-0.25, 0.25), -inf; 2: (0.25, 0.25), inf - inf = NaN; 3: (0, 0), 0 inf = NaN; 4 .. 7: seeded, whatever the signs give.  The DW3
    behind it takes |w| on the channels 0 and 1, so that their infinities keep the sign up to the pool"""
    import ref_global_desc as rg
    top = sorted(int(rg.prep(im, BATCH_WH[0], BATCH_WH[1])[0].max()) for im in imgs)
    t = top[0] + 1
    assert 1 < t <= top[1], top
    layers = batch_net(33, 65, relu6)
    prm = seeded(layers, seed)
    S = param_spans(layers)
    big = np.float32(3.0e38)
    w0 = prm[S[0][0]:S[0][1]].reshape(33, 3)
    w0[0] = (big, 0, 0)
    w0[1] = (-big, 0, 0)
    prm[S[0][1]:S[0][1] + 2] = 0
    w1 = prm[S[1][0]:S[1][1]].reshape(65, 33)
    w2 = prm[S[2][0]:S[2][1]].reshape(65, 9)
    pair = {0: (0.25, -0.25), 1: (-0.25, 0.25), 2: (0.25, 0.25), 3: (0.0, 0.0)}
    for co in range(65):
        if co % 8 in pair:
            w1[co, :2] = pair[co % 8]
        if co % 8 < 2:
            w2[co] = np.abs(w2[co])
    scale = float(np.finfo(np.float32).max) / 3.0e38 / (t - 0.5)
    return layers, prm, case_prep(BATCH_WH, mean=(0.0, 0.0, 0.0), scale=scale)


def float_classes(a):
    """share of zeros, subnormals, normals, infinities and NaNs among the floats of a"""
    m = bits(a).reshape(-1) & np.uint32(0x7FFFFFFF)
    n = float(max(m.size, 1))
    return dict(zero=(m == 0).sum() / n, subnormal=((m > 0) & (m < 0x00800000)).sum() / n,
                normal=((m >= 0x00800000) & (m < 0x7F800000)).sum() / n, inf=(m == 0x7F800000).sum() / n, nan=(m > 0x7F800000).sum() / n)


def chunks_of(njobs):
    """the sizes of the chunks the configured network (host build) splits a call of njobs into"""
    c = int(load_emu().emu_gd_chunk(int(njobs)))
    return [min(c, njobs - j0) for j0 in range(0, njobs, c)]


# ---- refusals of configure: name ->(layers, params transform, prep, words of the message) ----------------------------------------
def refusals():
    """[(name, kwargs of a refused configure, words, kwargs of the accepted neighbour)]; kwargs: layers, prep, mutate (on params), nparams"""
    good = tiny_net()[0]
    P = case_prep((16, 16))

    def sub(i, **kw):
        names = ("op", "cin", "cout", "stride", "relu6", "add_from")
        t = list(good)
        l = list(t[i])
        for k, v in kw.items():
            l[names.index(k)] = v
        t[i] = tuple(l)
        return t
    nan = lambda p: np.concatenate([[np.float32(np.nan)], p[1:]]).astype(np.float32)
    inf = lambda p: np.concatenate([p[:-1], [np.float32(np.inf)]]).astype(np.float32)
    big = lambda p: np.concatenate([[np.float32(3.0e38)], p[1:]]).astype(np.float32)
    R = [
        ("first_cin_not_3", dict(layers=[(CONV3, 4, 5, 2, 1, -1)] + good[1:]), "first layer's cin", dict(layers=good)),
        ("does_not_chain", dict(layers=sub(2, cin=6)), "does not chain", dict(layers=good)),
        ("dw_cin_ne_cout", dict(layers=[good[0], (DW3, 5, 6, 1, 1, -1), (PW, 6, 7, 1, 1, -1)] + good[3:]), "cin != cout", dict(layers=good)),
        ("stride_0", dict(layers=sub(0, stride=0)), "stride", dict(layers=sub(0, stride=1))),
        ("stride_3", dict(layers=sub(1, stride=3)), "stride", dict(layers=sub(1, stride=2))),
        ("add_from_self", dict(layers=sub(3, add_from=3)), "add_from", dict(layers=sub(3, add_from=1))),
        ("add_from_later", dict(layers=sub(3, add_from=4)), "add_from", dict(layers=sub(3, add_from=0))),
        ("add_from_below_minus_1", dict(layers=sub(3, add_from=-2)), "add_from", dict(layers=sub(3, add_from=-1))),
        ("add_from_other_shape", dict(layers=sub(3, add_from=2)), "add_from", dict(layers=sub(3, add_from=1))),
        ("add_from_with_relu6", dict(layers=sub(3, relu6=1)), "add_from", dict(layers=sub(3, relu6=0))),
        ("add_from_on_dw3", dict(layers=sub(1, add_from=0)), "add_from", dict(layers=sub(1, add_from=-1))),
        ("pool_missing", dict(layers=good[:-1]), "AVGPOOL", dict(layers=good)),
        ("pool_not_last", dict(layers=good[:2] + [(AVGPOOL, 5, 5, 1, 0, -1)] + good[2:]), "AVGPOOL", dict(layers=good)),
        ("dim_4097", dict(layers=pw_net(4, 4097)), "final dim", dict(layers=pw_net(4, 4096))),
        ("nparams_short", dict(layers=good, nparams=-1), "nparams", dict(layers=good)),
        ("nparams_long", dict(layers=good, nparams=+1), "nparams", dict(layers=good)),
        ("weight_nan", dict(layers=good, mutate=nan), "not finite", dict(layers=good, mutate=big)),
        ("bias_inf", dict(layers=good, mutate=inf), "not finite", dict(layers=good)),
        ("mean_nan", dict(layers=good, prep=case_prep((16, 16), mean=(0.5, float("nan"), 0.5))), "not finite", dict(layers=good)),
        ("scale_inf", dict(layers=good, prep=case_prep((16, 16), scale=float("inf"))), "not finite", dict(layers=good, prep=case_prep((16, 16), scale=3.0e38))),
        ("out_w_0", dict(layers=good, prep=case_prep((0, 16))), "below 1", dict(layers=good, prep=case_prep((1, 16)))),
        ("out_h_0", dict(layers=good, prep=case_prep((16, 0))), "below 1", dict(layers=good, prep=case_prep((16, 1)))),
    ]
    out = []
    for name, bad, words, ok in R:
        bad.setdefault("prep", P); ok.setdefault("prep", P)
        out.append((name, bad, words, ok))
    return out


def configure_args(kw, seed=5):
    """(layers, params, prep, nparams) of a refusal-table entry"""
    layers = kw["layers"]
    prm = seeded(layers, seed)
    if kw.get("mutate"):
        prm = kw["mutate"](prm)
    nparams = prm.size + kw["nparams"] if "nparams" in kw else prm.size
    if kw.get("nparams", 0) > 0:
        prm = np.concatenate([prm, np.zeros(kw["nparams"], np.float32)])
    return layers, prm, kw["prep"], nparams


# ---- the contexts these device tests make ---------------------------------------------------------------------------------------------
# The library deals its 16 pooled HIP streams to new contexts in rotation (pool_stream in csrc/svslam_hip.hip), and the runtime maps
# them onto a few hardware queues.  A test that times one context's call while another context's kernels hold the CUs
# (test_gpu_low_latency_pipeline.py) depends on the two landing on different queues, that is on how many contexts the process made
# before it.  So that these modules leave the rotation where they found it, every context they make is counted here and the last
# device test of the last module makes the rest of a multiple of 16 (small, closed at once).
ROTATION = 16
_made = [0]


def new_context(svs, *a, **kw):
    _made[0] += 1
    return svs.Context(*a, **kw)


def new_pipeline(pl, *a, **kw):
    """a pipeline of default_config (backend_on = 1) makes one context"""
    _made[0] += 1
    return pl.Pipeline(*a, **kw)


def settle_rotation(svs):
    """make and close the contexts that bring the count since the last call to a multiple of ROTATION; returns how many"""
    n = (-_made[0]) % ROTATION
    for _ in range(n):
        svs.Context(32, 32, max_slots=1, max_jobs=1).close()
    _made[0] = 0
    return n


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
