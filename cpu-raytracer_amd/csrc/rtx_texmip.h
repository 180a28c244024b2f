// rtx_texmip.h — rtx_update_texture on the device: a texture's level 0 converted from the caller's device buffer and its whole mip chain
// rebuilt in place, as HIP kernels for gfx950.  The arithmetic, the pass plan and the loops of a tile are rtx_texmip_math.h, which
// rtxh_texture_mips (the host twin) and texmip_check.cpp (the plan on the CPU, tile by tile) run too.
//
//   k_texmip<FORMAT>   one workgroup of 256 lanes per tile of the pass's source level (at most 32 x 32 texels, clipped to the level):
//                      the tile goes into LDS as planar r / g / b float arrays — the loads of a tile store to consecutive banks, and a lane's
//                      2 x 2 gather is dword reads at a stride of two dwords between lanes (two lanes of 32 on a bank at worst), where
//                      float4 texels would be 16-byte accesses at a stride of 32 bytes with a quarter of every access padding —
//                      pass 0 stores it as level 0 (one float4 per texel, w = 0, what the samplers load), and up to P halvings follow in
//                      LDS between two buffers, a barrier before each, every level stored as it is made.  A chain of 12 levels is 3
//                      launches at P = 5 instead of 11 at P = 1; the deeper levels of a tile are a quarter, a sixteenth, ... of its lanes.
//                      FORMAT: the caller's [h][w][3] f32 (three dword loads per texel: any 4-byte aligned address), the caller's
//                      [h][w][4] u8 through the 256-entry byte -> linear table made on the host (one dword load per texel, or four byte
//                      loads when the address is not 4-byte aligned; the table sits in LDS), or the chain's own float4 level (later passes).
// Every store is a vector store at an index computed from the block and lane index and the pass (host-made, from the validated shape):
// nothing is addressed through the caller's data.  No pointer and no DevTexture field changes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rtx_texmip_math.h"

enum { TEXMIP_RGB_F32 = RTX_TEXELS_RGB_F32, TEXMIP_RGBA8_SRGB = RTX_TEXELS_RGBA8_SRGB, TEXMIP_CHAIN = 2 };

struct TexSrcF32   { const float * p;   __device__ void load(int32_t at, float c[3]) const { const float * q = p + 3 * (size_t)at; c[0] = q[0]; c[1] = q[1]; c[2] = q[2]; } };
struct TexSrcChain { const float4 * p;  __device__ void load(int32_t at, float c[3]) const { const float4 v = p[at]; c[0] = v.x; c[1] = v.y; c[2] = v.z; } };
struct TexSrcRgba8 {
    const uint8_t * p; const float * lut; bool aligned;
    __device__ void load(int32_t at, float c[3]) const {
        const uint8_t * q = p + 4 * (size_t)at;
        uint32_t r, g, b;
        if (aligned) { const uint32_t v = *(const uint32_t *)q; r = v & 255u; g = (v >> 8) & 255u; b = (v >> 16) & 255u; }
        else { r = q[0]; g = q[1]; b = q[2]; }
        c[0] = lut[r]; c[1] = lut[g]; c[2] = lut[b];
    }
};
struct TexDstChain { float4 * p; __device__ void store(int32_t at, float r, float g, float b) { p[at] = make_float4(r, g, b, 0.0f); } };

template <int FORMAT>
__global__ __launch_bounds__(rtxt::BLOCK) void k_texmip(const rtxt::Pass pass, const void * __restrict__ src, float4 * __restrict__ chain, const float * __restrict__ lut) {
    __shared__ float a[3 * rtxt::PLANE_A];
    __shared__ float b[3 * rtxt::PLANE_B];
    __shared__ float s_lut[FORMAT == TEXMIP_RGBA8_SRGB ? 256 : 1];
    TexDstChain dst = { chain };
    const auto threads = [](auto && body) { body((int)threadIdx.x, (int)rtxt::BLOCK); };
    const auto sync = [] { __syncthreads(); };
    if constexpr (FORMAT == TEXMIP_RGB_F32) {
        const TexSrcF32 s = { (const float *)src };
        rtxt::tile_run(pass, (int32_t)blockIdx.x, s, dst, true, a, b, threads, sync);
    } else if constexpr (FORMAT == TEXMIP_RGBA8_SRGB) {
        s_lut[threadIdx.x] = lut[threadIdx.x];          // BLOCK = 256 = the table
        __syncthreads();
        const TexSrcRgba8 s = { (const uint8_t *)src, s_lut, ((uintptr_t)src & 3) == 0 };
        rtxt::tile_run(pass, (int32_t)blockIdx.x, s, dst, true, a, b, threads, sync);
    } else {
        const TexSrcChain s = { chain + pass.offset[0] };
        rtxt::tile_run(pass, (int32_t)blockIdx.x, s, dst, false, a, b, threads, sync);
    }
}
static_assert(rtxt::BLOCK == 256, "k_texmip<RGBA8> copies the 256-entry table with one lane per entry");
