// pyr_geom.h — where a pyramid level lies inside a slot.  Nothing of HIP in here: dev_common.h includes it for the kernels, a host
// emulation (tests/cpp/bm_host_emu) includes it after tests/cpp/hip_on_host.h and lays its images out the same way.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define SVS_BORDER 16          // stored REFLECT_101 border of every pyramid level
#define SVS_LEVELS 4

struct PyrGeom {
    int w[SVS_LEVELS], h[SVS_LEVELS];
    int pitch[SVS_LEVELS];          // bytes per padded row
    size_t ofs[SVS_LEVELS];         // byte offset of the padded level inside a slot
    size_t slot_bytes;
    int nlevels;
};

// pixel (0,0) of level l in a slot
__device__ __forceinline__ const uint8_t *lvl_origin(const uint8_t *slot, const PyrGeom &g, int l)
{
    return slot + g.ofs[l] + (size_t)SVS_BORDER * g.pitch[l] + SVS_BORDER;
}
__device__ __forceinline__ uint8_t *lvl_origin(uint8_t *slot, const PyrGeom &g, int l)
{
    return slot + g.ofs[l] + (size_t)SVS_BORDER * g.pitch[l] + SVS_BORDER;
}
