// csrc/k_colour.h compiled for the host (tests/test_host_emulation_colour.py): the HIP qualifiers vanish, a "thread" is a call of
// the per-thread function, a launch is the loop over the grid — including the threads past the last task, as the device runs them.
// The kernels of that file use no LDS and no cross-lane operation, so the emulation is a loop.  The 16-byte loads and stores are
// memcpy here; the source is copied into a heap block of exactly stride * (rows - 1) + 3 * src_w bytes first: the bytes the ABI
// promises to stay within, and no more.
#include "../hip_on_host.h"
static Dim3 threadIdx, blockIdx;
#include "../../../stereovision-slam_amd/csrc/k_colour.h"

// one image; src_w x src_h is w x h or halves to it.  grey: [h][w]; planes: [nplanes][h][w][3]; plane -1: none
extern "C" int emu_bgr_prepare(const uint8_t *src, int stride, int src_w, int src_h, int w, int h, int plane, uint8_t *grey, uint8_t *planes)
{
    const bool dec = src_w != w || src_h != h;
    const size_t bytes = (size_t)stride * (size_t)(src_h - 1) + 3 * (size_t)src_w;
    uint8_t *own = (uint8_t *)malloc(bytes);
    if (!own) return -1;
    memcpy(own, src, bytes);
    BgrJob jb;
    jb.src = own; jb.stride = col_row_stride(stride, dec); jb.plane = plane;
    const int chunks = col_chunks(w), nblk = (int)col_prepare_blocks(w, h);
    for (int t = 0; t < nblk * COL_THREADS; ++t) {
        if (dec) bgr_prepare_task<true>(jb, 0, t, w, h, src_w, chunks, grey, (size_t)w * h, planes);
        else bgr_prepare_task<false>(jb, 0, t, w, h, src_w, chunks, grey, (size_t)w * h, planes);
    }
    free(own);
    return 0;
}

extern "C" size_t emu_colour_bgr_per(int max_pts) { return col_bgr_per(max_pts); }

// n_points[njobs], plane_of[njobs], pix [njobs][max_pts], planes [nplanes][plane_bytes], out [njobs][out_per]
extern "C" int emu_colour_gather(int njobs, const int *n_points, const int *plane_of, const int *pix, int max_pts, const uint8_t *planes,
                                 size_t plane_bytes, uint8_t *out, size_t out_per)
{
    const int nblk = (int)col_gather_blocks(max_pts);
    for (int j = 0; j < njobs; ++j)
        for (int i = 0; i < nblk * COL_THREADS; ++i) colour_gather_task(j, i, n_points, 1, plane_of, pix, max_pts, planes, plane_bytes, out, out_per);
    return 0;
}
