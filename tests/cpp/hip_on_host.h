// Included before a kernel header of csrc/ that has no macro set of its own (k_cloud_filter.h, k_colour.h, k_stereo_bm.h) to compile
// it under g++: the HIP qualifiers vanish, min / max are the standard ones, atomicAdd is serial.  The index variables (Dim3) are the
// emulation's: statics where a "thread" is a call of the per-thread function, thread-local where real threads run a kernel (bm_host_emu).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
using std::min; using std::max;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct Dim3 { unsigned x, y, z; };
static inline unsigned atomicAdd(unsigned *p, unsigned v) { const unsigned o = *p; *p += v; return o; }
