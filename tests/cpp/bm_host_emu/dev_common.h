// Stand-in for csrc/dev_common.h when csrc/k_stereo_bm.h is compiled for the host (tests/test_host_emulation_stereo_bm.py): the HIP
// qualifiers vanish, threadIdx / blockIdx are per-thread variables, __syncthreads is a barrier of the workgroup's 256 host threads, LDS
// is the heap block g_lds, and the two gfx9 byte instructions the kernel uses are written out (v_alignbyte_b32: bytes sh..sh+3 of
// hi:lo; v_sad_u8: acc + the four absolute byte differences).  Level 0 of a slot is a bare w x h image here (no stored border).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include <algorithm>
#include <cstdlib>
using std::min; using std::max;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__
#define __launch_bounds__(x)
#define SVS_LEVELS 4
struct PyrGeom { int w[SVS_LEVELS], h[SVS_LEVELS]; int pitch[SVS_LEVELS]; size_t ofs[SVS_LEVELS]; size_t slot_bytes; int nlevels; };
static inline const uint8_t *lvl_origin(const uint8_t *slot, const PyrGeom &g, int l) { return slot + g.ofs[l]; }
struct Dim3 { unsigned x, y, z; };
extern thread_local Dim3 threadIdx, blockIdx;
extern Dim3 blockDim, gridDim;
extern unsigned int *g_lds;
void emu_barrier();
#define __syncthreads emu_barrier
static inline unsigned int emu_alignbyte(unsigned int hi, unsigned int lo, unsigned int sh) { return (unsigned int)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3))); }
static inline unsigned int emu_sad_u8(unsigned int a, unsigned int b, unsigned int acc) { for (int i = 0; i < 4; ++i) acc += (unsigned)std::abs((int)((a >> (8 * i)) & 255) - (int)((b >> (8 * i)) & 255)); return acc; }
#define __builtin_amdgcn_alignbyte emu_alignbyte
#define __builtin_amdgcn_sad_u8 emu_sad_u8
