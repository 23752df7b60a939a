// mesh_scan.h -- the wave64 / workgroup integer scan shared by mesh.hip and mesh_clean.hip (DPP row shifts and row broadcasts, the lane patterns
// of common.h's float scans).
#pragma once
#include "common.h"

namespace envgs {

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t mesh_dpp_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false); }

__device__ __forceinline__ uint32_t mesh_wave_scan_u32(uint32_t v)
{
    v += mesh_dpp_u32<0x111>(v); v += mesh_dpp_u32<0x112>(v); v += mesh_dpp_u32<0x114>(v); v += mesh_dpp_u32<0x118>(v);
    v += mesh_dpp_u32<0x142, 0xa>(v);
    v += mesh_dpp_u32<0x143, 0xc>(v);
    return v;
}

// exclusive prefix of v over the 256 threads of the workgroup (thread order) and the workgroup total; s_w: 4 words of LDS
__device__ __forceinline__ uint32_t mesh_block_exclusive(uint32_t v, uint32_t *s_w, uint32_t &total)
{
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint32_t inc = mesh_wave_scan_u32(v);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint32_t t = s_w[k]; all += t; before += (k < wave) ? t : 0u; }
    total = all;
    __syncthreads();
    return before + inc - v;
}

}  // namespace envgs
