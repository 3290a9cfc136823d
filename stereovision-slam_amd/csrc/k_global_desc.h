// Global image descriptor (svslam_gdesc_*): the network the reference runs on a keyframe's left image
// (LoopClosure::ExtractFeatureVec, src/loopclosure.cpp:92-129): a 7x7 Gaussian blur, a resize, blobFromImage, and MobileNetV2 up to the
// global average pool.  Here the network is a table of layers with hand-written kernels; the weights are an input.  All arithmetic of the
// layers is f32 and every output element is ONE chain in a fixed order, so that a VALU kernel, the f32-input MFMA and a plain C++ loop
// with std::fmaf give the same bits:
//   prep     integer blur (taps (8, 28, 56, 72, 56, 28, 8) / 256, horizontal sum kept in full, out = (v + 32768) >> 16, reflect-101),
//            integer bilinear resize (per-axis tables gd_axis, S = p[s] c0 + p[s + 1] c1, out = (((b0 (S0 >> 4)) >> 16) +
//            ((b1 (S1 >> 4)) >> 16) + 2) >> 2), x[c] = ((float)pix - mean[c]) * scale; planar CHW
//   CONV3    acc = bias[co]; acc = fmaf(w, x, acc) over (ci, ky, kx) row-major, a tap in the padding takes x = +0.0f
//   DW3      acc = bias[c]; the 9 taps in (ky, kx) order, padding as above
//   PW       acc = bias[co]; acc = fmaf(w[co][ci], x[ci], acc), ci ascending
//   AVGPOOL  s = +0; s = s + x over the pixels in row-major order; s / (float)(H W)
//   epilogue v = acc (+ the output of layer add_from, one f32 add); ReLU6 is v = v > 0 ? v : +0, then v = v < 6 ? v : 6 (fminf(fmaxf(v, 0), 6)
//            with the sign of a zero and a NaN pinned)
// Activations are planar [C][H W] f32 per job; a job's layers live at fixed offsets (gd_plan_buffers: first fit over the outputs'
// lifetimes) of its share of the workspace, the jobs of a chunk one share after the other.
// Kernels: k_gd_prep, k_gd_conv3, k_gd_dw3, k_gd_pool and the VALU k_gd_pw take one output element per thread.  k_gd_pw_mfma is PW on
// v_mfma_f32_32x32x2_f32: a wave owns 32 pixels (of the chunk's jobs laid end to end) x up to 128 output channels, up to four
// accumulators initialised to the bias, A = the weights transposed and padded to 32 channels on the device ([ci][coutp], so 32 lanes read 32
// neighbouring floats), B = the activations.  A tap beyond cin (odd cin) is a = -0.0f, b = +0.0f: its product -0 leaves every
// accumulator, +0 and -0 included, as it is.
// The file is plain C++ between the HIP qualifiers: compiled for the host with GD_HOST_EMU (tests/cpp/gd_host_emu) an element function
// is called in a loop and fmaf is std::fmaf.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define GD_CONV3 0
#define GD_DW3 1
#define GD_PW 2
#define GD_AVGPOOL 3
#define GD_MAX_DIM 4096                       // the loop store's limit
#define GD_THREADS 256
#define GD_DEFAULT_WORKSPACE ((long long)256 << 20)

#ifdef GD_HOST_EMU
#include <cmath>
#define GD_DEV static inline
#define GD_FMA(a, b, c) std::fmaf((a), (b), (c))
#else
#define GD_DEV __device__ __forceinline__
#define GD_FMA(a, b, c) fmaf((a), (b), (c))
#endif

struct GdLayer { int op, cin, cout, stride, relu6, add_from; };
struct GdPrep { int out_w, out_h; float mean[3]; float scale; long long workspace_bytes; };

// a layer as the kernels take it; offsets in floats: w / b into the packed parameters, in / out / res into a job's share
struct GdL {
    int op, cin, cout, stride, relu6, add_from;
    int hin, win, hout, wout, coutp, pad;
    long long w, b, in, out, res;
};

struct GdNet {
    std::vector<GdL> L;
    std::vector<float> packed;             // the parameters in the kernels' layout
    std::vector<int> tab;                  // [xs | xs1 | xc0 | xc1] (out_w each) [ys | ys1 | yc0 | yc1] (out_h each)
    GdPrep prep;
    int src_w = 0, src_h = 0, dim = 0;
    long long job_floats = 0;              // a job's share of the workspace
};

// level 0 of the slots as the kernels read it: pixel (x, y) of slot s is base[s * slot_bytes + origin + y * pitch + x]
struct GdImg { const uint8_t *base; size_t slot_bytes, origin; int pitch, w, h; };

struct GdPrepArgs {
    GdImg I;
    const int *slots;                      // [njobs of the chunk]
    const int *tab;
    float *ws;                             // the chunk's workspace; the blob of job j is ws + j * job_floats (offset 0)
    uint8_t *u8;                           // host build only: the resized image [job][out_h][out_w], or null
    long long job_floats;
    int out_w, out_h, njobs;
    float mean[3], scale;
};

struct GdArgs {                            // one layer over the jobs of a chunk
    GdL L;
    const float *prm;
    float *ws;
    float *vecs;                           // AVGPOOL: [njobs][cout]
    long long job_floats;
    int njobs;
};

static inline long long gd_param_count(const GdLayer &l)
{
    if (l.op == GD_CONV3) return (long long)l.cout * l.cin * 9 + l.cout;
    if (l.op == GD_DW3) return (long long)l.cout * 9 + l.cout;
    if (l.op == GD_PW) return (long long)l.cout * l.cin + l.cout;
    return 0;
}

// MobileNetV2 up to the global average pool: 52 convolutions + the pool.  Returns the count; writes min(count, cap) entries.
static inline int gd_mobilenet_v2(GdLayer *out, int cap)
{
    std::vector<GdLayer> T;
    T.push_back(GdLayer{ GD_CONV3, 3, 32, 2, 1, -1 });
    static const int cfg[7][4] = { { 1, 16, 1, 1 }, { 6, 24, 2, 2 }, { 6, 32, 3, 2 }, { 6, 64, 4, 2 }, { 6, 96, 3, 1 }, { 6, 160, 3, 2 }, { 6, 320, 1, 1 } };
    int cin = 32;
    for (int g = 0; g < 7; ++g)
        for (int i = 0; i < cfg[g][2]; ++i) {
            const int t = cfg[g][0], c = cfg[g][1], s = i == 0 ? cfg[g][3] : 1, hid = cin * t;
            const int from = (int)T.size() - 1;                     // the layer whose output enters the block
            if (t != 1) T.push_back(GdLayer{ GD_PW, cin, hid, 1, 1, -1 });
            T.push_back(GdLayer{ GD_DW3, hid, hid, s, 1, -1 });
            T.push_back(GdLayer{ GD_PW, hid, c, 1, 0, (s == 1 && cin == c) ? from : -1 });
            cin = c;
        }
    T.push_back(GdLayer{ GD_PW, 320, 1280, 1, 1, -1 });
    T.push_back(GdLayer{ GD_AVGPOOL, 1280, 1280, 1, 0, -1 });
    for (int i = 0; i < (int)T.size() && i < cap; ++i) out[i] = T[(size_t)i];
    return (int)T.size();
}

static inline GdPrep gd_default_prep()
{
    GdPrep p;
    p.out_w = 224; p.out_h = 224;
    p.mean[0] = 0.485f; p.mean[1] = 0.456f; p.mean[2] = 0.406f;
    p.scale = (float)(1.0 / 255.0);
    p.workspace_bytes = 0;
    return p;
}

static inline bool gd_finite(float v) { return v == v && fabsf(v) <= 3.4028234663852886e38f; }

// one axis of the resize: first tap, second tap (clamped) and the two coefficients of destination index d
static inline void gd_axis(int src, int dst, int *s0, int *s1, int *c0, int *c1)
{
    const double scale = (double)src / (double)dst;
    for (int d = 0; d < dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= (float)s;
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= src - 1) { s = src - 1; f = 0.f; }
        s0[d] = s; s1[d] = s + 1 < src ? s + 1 : src - 1;
        const float one_minus = 1.f - f;
        c0[d] = (int)(short)nearbyintf(one_minus * 2048.f);
        c1[d] = (int)(short)nearbyintf(f * 2048.f);
    }
}

// returns nullptr or the reason the configuration is refused; N is filled only on success (it is a fresh object either way)
static inline const char *gd_configure(GdNet &N, int src_w, int src_h, int nlayers, const GdLayer *layers, const float *params, long long nparams,
                                       const GdPrep *prep_in)
{
    const GdPrep P = prep_in ? *prep_in : gd_default_prep();
    if (nlayers < 1 || !layers) return "an empty table";
    if (nlayers > 4096) return "more than 4096 layers";
    if (P.out_w < 1 || P.out_h < 1) return "out_w or out_h is below 1";
    if (P.out_w > 4096 || P.out_h > 4096) return "out_w or out_h is above 4096";
    if (!gd_finite(P.mean[0]) || !gd_finite(P.mean[1]) || !gd_finite(P.mean[2]) || !gd_finite(P.scale)) return "mean or scale is not finite";
    if (P.workspace_bytes < 0) return "workspace_bytes is negative";
    long long total = 0;
    int c = 3, h = P.out_h, w = P.out_w;
    std::vector<GdL> L((size_t)nlayers);
    for (int i = 0; i < nlayers; ++i) {
        const GdLayer &l = layers[i];
        GdL &o = L[(size_t)i];
        if (l.op < GD_CONV3 || l.op > GD_AVGPOOL) return "an unknown op";
        if (l.cin != c) return i == 0 ? "the first layer's cin is not 3" : "the table does not chain (cin is not the previous cout)";
        if (l.cout < 1 || l.cout > (1 << 16)) return "cout outside 1 .. 65536";
        if ((l.op == GD_DW3 || l.op == GD_AVGPOOL) && l.cin != l.cout) return "DW3 or AVGPOOL with cin != cout";
        if (l.op == GD_AVGPOOL && i != nlayers - 1) return "AVGPOOL is not the last layer";
        if (l.op != GD_AVGPOOL && i == nlayers - 1) return "the last layer is not AVGPOOL";
        if ((l.op == GD_CONV3 || l.op == GD_DW3) && l.stride != 1 && l.stride != 2) return "a stride outside {1, 2}";
        if (l.add_from < -1) return "a bad add_from";
        o.op = l.op; o.cin = l.cin; o.cout = l.cout; o.stride = (l.op == GD_CONV3 || l.op == GD_DW3) ? l.stride : 1; o.relu6 = l.relu6 ? 1 : 0;
        o.add_from = l.add_from; o.hin = h; o.win = w; o.pad = 0;
        if (l.op == GD_CONV3 || l.op == GD_DW3) { h = (h + 2 - 3) / o.stride + 1; w = (w + 2 - 3) / o.stride + 1; }
        if (l.op == GD_AVGPOOL) { h = 1; w = 1; }
        if (h < 1 || w < 1) return "a map shrinks to 0";
        o.hout = h; o.wout = w; o.coutp = (l.cout + 31) & ~31;
        if (l.add_from >= 0) {
            if (l.op != GD_PW || l.relu6) return "a bad add_from (only on PW with relu6 == 0)";
            if (l.add_from >= i) return "a bad add_from (not an earlier layer)";
            const GdL &r = L[(size_t)l.add_from];
            if (r.op == GD_AVGPOOL || r.cout != l.cout || r.hout != h || r.wout != w) return "a bad add_from (another C x H x W)";
        }
        c = l.cout;
        total += gd_param_count(l);
    }
    if (c < 1 || c > GD_MAX_DIM) return "the final dim is outside 1 .. 4096";
    if (nparams != total) return "nparams is not the table's total";
    if (total && !params) return "null params";
    for (long long i = 0; i < total; ++i) if (!gd_finite(params[i])) return "a weight is not finite";

    // the parameters in the kernels' layout: PW transposed [cin][coutp] + bias[coutp]; the others as given
    std::vector<float> packed;
    const float *p = params;
    for (int i = 0; i < nlayers; ++i) {
        GdL &o = L[(size_t)i];
        const long long nw = gd_param_count(layers[i]) - (o.op == GD_AVGPOOL ? 0 : o.cout);
        o.w = (long long)packed.size();
        if (o.op == GD_PW) {
            packed.resize(packed.size() + (size_t)o.cin * o.coutp + o.coutp, 0.f);
            float *wt = packed.data() + o.w;
            for (int co = 0; co < o.cout; ++co)
                for (int ci = 0; ci < o.cin; ++ci) wt[(size_t)ci * o.coutp + co] = p[(size_t)co * o.cin + ci];
            o.b = o.w + (long long)o.cin * o.coutp;
            memcpy(packed.data() + o.b, p + nw, sizeof(float) * (size_t)o.cout);
        } else if (o.op != GD_AVGPOOL) {
            packed.insert(packed.end(), p, p + nw + o.cout);
            o.b = o.w + nw;
        } else o.b = o.w;
        p += gd_param_count(layers[i]);
        while (packed.size() & 31) packed.push_back(0.f);
    }

    // buffers: the blob is "layer -1" at offset 0; output i lives from layer i to its last reader; first fit, lowest offset
    struct Live { long long off, size; int last; };
    std::vector<Live> live;
    std::vector<int> last((size_t)nlayers, 0);
    for (int i = 0; i < nlayers; ++i) { last[(size_t)i] = i + 1; }
    for (int i = 0; i < nlayers; ++i) if (L[(size_t)i].add_from >= 0 && last[(size_t)L[(size_t)i].add_from] < i) last[(size_t)L[(size_t)i].add_from] = i;
    std::vector<long long> off((size_t)nlayers, 0);
    long long peak = ((long long)3 * P.out_h * P.out_w + 63) & ~63LL;
    live.push_back(Live{ 0, peak, 0 });
    for (int i = 0; i + 1 < nlayers; ++i) {                      // the pool writes to the call's vectors, not to the workspace
        const GdL &o = L[(size_t)i];
        const long long size = ((long long)o.cout * o.hout * o.wout + 63) & ~63LL;
        for (size_t k = 0; k < live.size();) { if (live[k].last < i) live.erase(live.begin() + (long)k); else ++k; }
        long long best = -1;
        for (size_t cand = 0; cand <= live.size(); ++cand) {
            const long long at = cand == 0 ? 0 : live[cand - 1].off + live[cand - 1].size;
            bool ok = true;
            for (const Live &v : live) if (at < v.off + v.size && v.off < at + size) { ok = false; break; }
            if (ok && (best < 0 || at < best)) best = at;
        }
        off[(size_t)i] = best;
        live.push_back(Live{ best, size, last[(size_t)i] });
        if (best + size > peak) peak = best + size;
    }
    for (int i = 0; i < nlayers; ++i) {
        GdL &o = L[(size_t)i];
        o.in = i == 0 ? 0 : off[(size_t)i - 1];
        o.out = off[(size_t)i];
        o.res = o.add_from >= 0 ? off[(size_t)o.add_from] : 0;
    }
    if (peak > ((long long)1 << 40)) return "a job's activations pass 2^40 floats";

    N.L.swap(L); N.packed.swap(packed);
    N.prep = P; N.src_w = src_w; N.src_h = src_h; N.dim = c; N.job_floats = peak;
    N.tab.assign((size_t)4 * P.out_w + 4 * P.out_h, 0);
    if (src_w >= 1 && src_h >= 1) {
        int *t = N.tab.data();
        gd_axis(src_w, P.out_w, t, t + P.out_w, t + 2 * P.out_w, t + 3 * P.out_w);
        t += 4 * P.out_w;
        gd_axis(src_h, P.out_h, t, t + P.out_h, t + 2 * P.out_h, t + 3 * P.out_h);
    }
    return nullptr;
}

// jobs per chunk under the workspace's cap; never below one (a cap below one job's share still runs one job at a time)
static inline int gd_chunk(const GdNet &N, int njobs)
{
    const long long cap = N.prep.workspace_bytes > 0 ? N.prep.workspace_bytes : GD_DEFAULT_WORKSPACE;
    long long n = cap / (4 * N.job_floats);
    if (n < 1) n = 1;
    if (n > 8192) n = 8192;                                       // a grid dimension
    return n < njobs ? (int)n : njobs;
}

// k_gd_pw_mfma's channel tiles per wave for a PW layer of hw pixels per job over the nj jobs of a chunk: four while that leaves 2048
// waves (two per SIMD of the chip's 256 CUs), else fewer
static inline int gd_pw_tiles(long long hw, int nj, int coutp)
{
    const long long ptiles = (hw * nj + 31) / 32;
    const int ct = coutp / 32;
    int NT = 4;
    while (NT > 1 && ptiles * ((ct + NT - 1) / NT) < 2048) NT >>= 1;
    return NT;
}

static inline const char *gd_check_describe(const GdNet &N, int njobs, const int *slots, int nslots)
{
    if (N.dim == 0) return "no network is configured";
    if (N.src_w < 4 || N.src_h < 4) return "the image is below 4 x 4";
    for (int j = 0; j < njobs; ++j) if (slots[j] < 0 || slots[j] >= nslots) return "a slot is out of range";
    return nullptr;
}

// ---- prep: one output pixel -------------------------------------------------------------------------------------------------------
GD_DEV int gd_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// the blurred pixel (x, y): 7 horizontal sums, then the vertical one
GD_DEV int gd_blur_at(const uint8_t *img, int pitch, int w, int h, int x, int y)
{
    const int x0 = gd_reflect(x - 3, w), x1 = gd_reflect(x - 2, w), x2 = gd_reflect(x - 1, w), x4 = gd_reflect(x + 1, w), x5 = gd_reflect(x + 2, w),
              x6 = gd_reflect(x + 3, w);
    const int tap[7] = { 8, 28, 56, 72, 56, 28, 8 };
    int v = 0;
    for (int k = 0; k < 7; ++k) {
        const uint8_t *p = img + (size_t)gd_reflect(y - 3 + k, h) * pitch;
        const int hs = 8 * ((int)p[x0] + (int)p[x6]) + 28 * ((int)p[x1] + (int)p[x5]) + 56 * ((int)p[x2] + (int)p[x4]) + 72 * (int)p[x];
        v += tap[k] * hs;
    }
    return (v + 32768) >> 16;
}

GD_DEV void gd_prep_elem(const GdPrepArgs &A, int job, int oy, int ox)
{
    const uint8_t *img = A.I.base + (size_t)A.slots[job] * A.I.slot_bytes + A.I.origin;
    const int *xt = A.tab, *yt = A.tab + 4 * A.out_w;
    const int sx0 = xt[ox], sx1 = xt[A.out_w + ox], a0 = xt[2 * A.out_w + ox], a1 = xt[3 * A.out_w + ox];
    const int sy0 = yt[oy], sy1 = yt[A.out_h + oy], b0 = yt[2 * A.out_h + oy], b1 = yt[3 * A.out_h + oy];
    const int p00 = gd_blur_at(img, A.I.pitch, A.I.w, A.I.h, sx0, sy0), p01 = gd_blur_at(img, A.I.pitch, A.I.w, A.I.h, sx1, sy0);
    const int p10 = gd_blur_at(img, A.I.pitch, A.I.w, A.I.h, sx0, sy1), p11 = gd_blur_at(img, A.I.pitch, A.I.w, A.I.h, sx1, sy1);
    const int S0 = p00 * a0 + p01 * a1, S1 = p10 * a0 + p11 * a1;
    const int pix = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
    const size_t plane = (size_t)A.out_w * A.out_h, at = (size_t)oy * A.out_w + ox;
    float *blob = A.ws + (size_t)job * A.job_floats;
    const float fp = (float)pix;
    for (int c = 0; c < 3; ++c) {
        const float d = fp - A.mean[c];
        blob[(size_t)c * plane + at] = d * A.scale;
    }
    if (A.u8) A.u8[(size_t)job * plane + at] = (uint8_t)(pix < 0 ? 0 : (pix > 255 ? 255 : pix));
}

// ---- layers: one output element ---------------------------------------------------------------------------------------------------
GD_DEV float gd_epilogue(const GdArgs &A, const float *jw, float acc, int co, int pix)
{
    float v = acc;
    if (A.L.add_from >= 0) v = v + jw[A.L.res + (long long)co * A.L.hout * A.L.wout + pix];
    if (A.L.relu6) { v = v > 0.f ? v : 0.f; v = v < 6.f ? v : 6.f; }
    return v;
}

GD_DEV void gd_conv3_elem(const GdArgs &A, int job, int co, int pix)
{
    const GdL &L = A.L;
    float *jw = A.ws + (size_t)job * A.job_floats;
    const float *x = jw + L.in, *w = A.prm + L.w + (size_t)co * L.cin * 9;
    const int oy = pix / L.wout, ox = pix - oy * L.wout, iy0 = oy * L.stride - 1, ix0 = ox * L.stride - 1;
    float acc = A.prm[L.b + co];
    for (int ci = 0; ci < L.cin; ++ci) {
        const float *xc = x + (size_t)ci * L.hin * L.win;
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = iy0 + ky, ix = ix0 + kx;
                const float xv = (iy >= 0 && iy < L.hin && ix >= 0 && ix < L.win) ? xc[(size_t)iy * L.win + ix] : 0.f;
                acc = GD_FMA(w[ci * 9 + ky * 3 + kx], xv, acc);
            }
    }
    jw[L.out + (size_t)co * L.hout * L.wout + pix] = gd_epilogue(A, jw, acc, co, pix);
}

GD_DEV void gd_dw3_elem(const GdArgs &A, int job, int c, int pix)
{
    const GdL &L = A.L;
    float *jw = A.ws + (size_t)job * A.job_floats;
    const float *xc = jw + L.in + (size_t)c * L.hin * L.win, *w = A.prm + L.w + (size_t)c * 9;
    const int oy = pix / L.wout, ox = pix - oy * L.wout, iy0 = oy * L.stride - 1, ix0 = ox * L.stride - 1;
    float acc = A.prm[L.b + c];
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            const int iy = iy0 + ky, ix = ix0 + kx;
            const float xv = (iy >= 0 && iy < L.hin && ix >= 0 && ix < L.win) ? xc[(size_t)iy * L.win + ix] : 0.f;
            acc = GD_FMA(w[ky * 3 + kx], xv, acc);
        }
    jw[L.out + (size_t)c * L.hout * L.wout + pix] = gd_epilogue(A, jw, acc, c, pix);
}

GD_DEV void gd_pw_elem(const GdArgs &A, int job, int co, int pix)
{
    const GdL &L = A.L;
    float *jw = A.ws + (size_t)job * A.job_floats;
    const size_t hw = (size_t)L.hout * L.wout;
    const float *x = jw + L.in + pix, *wt = A.prm + L.w + co;
    float acc = A.prm[L.b + co];
    for (int ci = 0; ci < L.cin; ++ci) acc = GD_FMA(wt[(size_t)ci * L.coutp], x[(size_t)ci * hw], acc);
    jw[L.out + (size_t)co * hw + pix] = gd_epilogue(A, jw, acc, co, pix);
}

GD_DEV void gd_pool_elem(const GdArgs &A, int job, int c)
{
    const GdL &L = A.L;
    const int hw = L.hin * L.win;
    const float *x = A.ws + (size_t)job * A.job_floats + L.in + (size_t)c * hw;
    float s = 0.f;
    for (int i = 0; i < hw; ++i) s = s + x[i];
    A.vecs[(size_t)job * L.cout + c] = s / (float)hw;
}

#ifndef GD_HOST_EMU
__global__ void __launch_bounds__(GD_THREADS) k_gd_prep(GdPrepArgs A)
{
    const int i = (int)(blockIdx.x * GD_THREADS + threadIdx.x), job = (int)blockIdx.y;
    if (i >= A.out_w * A.out_h) return;
    gd_prep_elem(A, job, i / A.out_w, i % A.out_w);
}

// grid (ceil(pixels / 256), cout, jobs)
__global__ void __launch_bounds__(GD_THREADS) k_gd_conv3(GdArgs A)
{
    const int pix = (int)(blockIdx.x * GD_THREADS + threadIdx.x);
    if (pix >= A.L.hout * A.L.wout) return;
    gd_conv3_elem(A, (int)blockIdx.z, (int)blockIdx.y, pix);
}

// grid (ceil(c * pixels / 256), jobs)
__global__ void __launch_bounds__(GD_THREADS) k_gd_dw3(GdArgs A)
{
    const long long i = (long long)blockIdx.x * GD_THREADS + threadIdx.x;
    const int hw = A.L.hout * A.L.wout;
    if (i >= (long long)A.L.cout * hw) return;
    gd_dw3_elem(A, (int)blockIdx.y, (int)(i / hw), (int)(i % hw));
}

// the VALU form of PW: grid (ceil(cout * pixels / 256), jobs)
__global__ void __launch_bounds__(GD_THREADS) k_gd_pw(GdArgs A)
{
    const long long i = (long long)blockIdx.x * GD_THREADS + threadIdx.x;
    const int hw = A.L.hout * A.L.wout;
    if (i >= (long long)A.L.cout * hw) return;
    gd_pw_elem(A, (int)blockIdx.y, (int)(i / hw), (int)(i % hw));
}

// grid (ceil(cout / 256), jobs)
__global__ void __launch_bounds__(GD_THREADS) k_gd_pool(GdArgs A)
{
    const int c = (int)(blockIdx.x * GD_THREADS + threadIdx.x);
    if (c >= A.L.cout) return;
    gd_pool_elem(A, (int)blockIdx.y, c);
}

// PW on the f32-input MFMA.  grid (ceil(njobs * pixels / 128), ceil(coutp / (32 NT))); wave v of a workgroup owns pixels
// (4 blockIdx.x + v) * 32 .. + 31 of the chunk's jobs laid end to end, and channels 32 NT blockIdx.y .. in NT 32 x 32 tiles (the host
// takes NT = 4 when that still fills the chip and fewer tiles per wave otherwise; an output's chain does not depend on it).
// Lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31]; register i of an accumulator is row (i & 3) + 8 (i >> 2) +
// 4 (l >> 5), column l & 31.  Nothing crosses waves: no LDS, no barrier.  The channel loop takes GD_PW_U steps (2 GD_PW_U channels) at
// a time: all their loads are issued before the first MFMA, which then run in channel order.  A tile beyond coutp (last group only)
// and a pixel beyond the chunk compute on valid addresses (tile 0, pixel 0 of job 0) and are not stored.
#define GD_PW_U 4
typedef float gd_f32x16 __attribute__((ext_vector_type(16)));
template <int NT> __global__ void __launch_bounds__(GD_THREADS) k_gd_pw_mfma(GdArgs A)
{
    const GdL &L = A.L;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int hw = L.hout * L.wout;
    const long long npix = (long long)A.njobs * hw, n = ((long long)blockIdx.x * 4 + wave) * 32 + r;
    if (n - r >= npix) return;                                   // the whole wave
    const bool valid = n < npix;
    const int job = valid ? (int)(n / hw) : 0, pix = valid ? (int)(n - (long long)job * hw) : 0;
    float *jw = A.ws + (size_t)job * A.job_floats;
    const float *xb = jw + L.in + pix + (size_t)h * hw;          // this lane's k is even k + h
    const int co0 = (int)blockIdx.y * 32 * NT;
    const int nt = (L.coutp - co0) / 32 < NT ? (L.coutp - co0) / 32 : NT;    // tiles of this wave, uniform
    const float *wt = A.prm + L.w + co0 + r + (size_t)h * L.coutp, *bias = A.prm + L.b + co0;
    int tofs[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) tofs[t] = t < nt ? 32 * t : 0;
    gd_f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = bias[tofs[t] + (i & 3) + 8 * (i >> 2) + 4 * h];
    int k0 = 0;
    for (; k0 + 2 * GD_PW_U <= L.cin; k0 += 2 * GD_PW_U) {
        float b[GD_PW_U], a[GD_PW_U][NT];
#pragma unroll
        for (int u = 0; u < GD_PW_U; ++u) {
            b[u] = xb[(size_t)(k0 + 2 * u) * hw];
            const float *wk = wt + (size_t)(k0 + 2 * u) * L.coutp;
#pragma unroll
            for (int t = 0; t < NT; ++t) a[u][t] = wk[tofs[t]];
        }
#pragma unroll
        for (int u = 0; u < GD_PW_U; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][t], b[u], acc[t], 0, 0, 0);
    }
    for (; k0 < L.cin; k0 += 2) {                                // the last channels, one step at a time
        const bool inb = k0 + h < L.cin;
        const float *xk = inb ? xb + (size_t)k0 * hw : jw + L.in;             // beyond cin: any valid address, the value is not used
        const float *wk = inb ? wt + (size_t)k0 * L.coutp : A.prm + L.w + co0 + r;
        const float b = inb ? xk[0] : 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float a = inb ? wk[tofs[t]] : -0.f;
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
        }
    }
    if (!valid) return;
#pragma unroll
    for (int t = 0; t < NT; ++t)
        if (t < nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = co0 + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (co < L.cout) jw[L.out + (size_t)co * hw + pix] = gd_epilogue(A, jw, acc[t][i], co, pix);
            }
}
#endif
