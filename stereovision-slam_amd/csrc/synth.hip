// synth.hip — HIP generator of the synthetic stereo stream (bench / test input,
// rendered straight into HBM so the timed region starts with resident frames).
// Input generation only; not part of the hot path.
#include <hip/hip_runtime.h>
#include "synth_scene.h"

__global__ void __launch_bounds__(256)
k_synth_render(const svs_synth_view *views, int w, int h, uint8_t *out)
{
    const svs_synth_view v = views[blockIdx.z];
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= w || y >= h) return;
    out[(size_t)blockIdx.z * w * h + (size_t)y * w + x] = svs_synth_pixel(&v, x, y);
}

// The fused 1/2 nearest decimation of the pyramid (k_pyr_fused) uses only the pixels (2x, 2y) of a full-size frame.  This
// variant ray-casts just those pixels and writes each into its 2x2 block: the decimated image is bit-identical to that of a
// full render, at a quarter of the per-pixel work.
__global__ void __launch_bounds__(256)
k_synth_render_sampled(const svs_synth_view *views, int w, int h, uint8_t *out)
{
    const svs_synth_view v = views[blockIdx.z];
    const int x = 2 * (blockIdx.x * blockDim.x + threadIdx.x);
    const int y = 2 * (blockIdx.y * blockDim.y + threadIdx.y);
    if (x >= w || y >= h) return;
    const uint8_t p = svs_synth_pixel(&v, x, y);
    uint8_t *o = out + (size_t)blockIdx.z * w * h + (size_t)y * w + x;
    const bool right = x + 1 < w, below = y + 1 < h;
    o[0] = p;
    if (right) o[1] = p;
    if (below) o[w] = p;
    if (right && below) o[w + 1] = p;
}

static int render_batch(int device, int n, const svs_synth_view *views, int w, int h, void *d_out, bool sampled)
{
    if (n <= 0) return 0;
    if (hipSetDevice(device) != hipSuccess) return -1;
    svs_synth_view *dv = nullptr;
    if (hipMalloc(&dv, sizeof(svs_synth_view) * n) != hipSuccess) return -2;
    int rc = 0;
    if (hipMemcpy(dv, views, sizeof(svs_synth_view) * n, hipMemcpyHostToDevice) != hipSuccess) rc = -3;
    if (!rc) {
        dim3 blk(64, 4);
        if (sampled) {
            const int sw = (w + 1) / 2, sh = (h + 1) / 2;
            hipLaunchKernelGGL(k_synth_render_sampled, dim3((sw + 63) / 64, (sh + 3) / 4, n), blk, 0, 0, dv, w, h,
                               static_cast<uint8_t *>(d_out));
        } else {
            hipLaunchKernelGGL(k_synth_render, dim3((w + 63) / 64, (h + 3) / 4, n), blk, 0, 0, dv, w, h,
                               static_cast<uint8_t *>(d_out));
        }
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -4;
    }
    (void)hipFree(dv);
    return rc;
}

extern "C" int svslam_synth_render_batch(int device, int n, const svs_synth_view *views, int w, int h,
                                         void *d_out)
{
    return render_batch(device, n, views, w, h, d_out, false);
}

// the pixels the 1/2 nearest decimation samples, each replicated into its 2x2 block (k_synth_render_sampled)
extern "C" int svslam_synth_render_batch_sampled(int device, int n, const svs_synth_view *views, int w, int h,
                                                 void *d_out)
{
    return render_batch(device, n, views, w, h, d_out, true);
}
