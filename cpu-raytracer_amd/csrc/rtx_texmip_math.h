// rtx_texmip_math.h — the shape, the box filter and the pass plan of a texture's mip chain (Texture::load, Texture.cpp:49-55, 76-117), written
// once and compiled three times like rtx_refit_math.h: by hipcc into the kernels of rtx_texmip.h (rtx_update_texture), by the host compiler
// into rtxh_texture_mips (host/rtx_host.cpp), the specification the device chain is compared with, and into texmip_check.cpp, which runs the
// pass plan tile by tile on the CPU.  No HIP in it.
//
//   chain_shape   the descriptor Texture::load gives a width x height image: a chain of 1 + (int)log2f(min(w, h)) levels when it is asked
//                 for and both sides are powers of two, level l (w >> l) x (h >> l) texels at the cumulative offset; one level otherwise
//   box           one texel of a level from the 2 x 2 texels of the level before: (((c0 + c1) + c2) + c3) * 0.25f per channel, c0 = (2i, 2j),
//                 c1 = (2i + 1, 2j), c2 = (2i, 2j + 1), c3 = (2i + 1, 2j + 1) (Texture.cpp:99-104).  Unfused fp32 adds and one multiply by a
//                 power of two: the same bits on both sides for every float (a NaN stays a NaN, its sign and payload are not pinned)
//   plan_passes   which launches rewrite a chain.  A pass reads one SOURCE level in tiles of at most TILE x TILE texels, clipped to the
//                 level, and makes up to P levels below it; the next pass starts from the last level written.  Pass 0 reads the caller's
//                 buffer and also stores level 0.  P = 1 is one launch per level.
//   tile_load / tile_reduce   what one workgroup does with its tile, as loops over (thread, thread count): the kernel runs them with its
//                 threads and a barrier in between, texmip_check.cpp with a loop over the threads.  Texels come from a Src and go to a
//                 Dst (the caller's buffer, the chain; on the CPU counting stand-ins), the tile itself lives in planar r / g / b arrays.
// Why a tile reduces on its own: a chain only exists for powers of two, so a tile of a chained level is 2^a x 2^b texels at a multiple of
// TILE, and k <= min(a, b) halvings of it are exactly the texels [x0 >> k, (x0 + w) >> k) x [y0 >> k, (y0 + h) >> k) of level + k.
#pragma once
#include <stdint.h>
#include <math.h>
#include "../../include/rtx.h"

#if !defined(RTX_HD)
#if defined(__HIPCC__)
#define RTX_HD __host__ __device__ inline
#else
#define RTX_HD inline
#endif
#endif

namespace rtxt {

enum { TILE = 32, MAX_PASS_LEVELS = 5, BLOCK = 256,       // BLOCK: a multiple of TILE (tile_load)
       DEFAULT_PASS_LEVELS = 5,                              // RTX_TEX_PASS_LEVELS when it is not set: measured against 1, a launch per level
       PLANE_A = TILE * TILE, PLANE_B = (TILE / 2) * (TILE / 2) };      // floats per colour plane of the two tile buffers a reduction alternates between

// desc and texel_count for a width x height texture (both >= 1).  RTX_ERR_LIMIT: more than RTX_MAX_MIP_LEVELS levels, or a texel count
// beyond the int32_t offsets of the descriptor; desc is then not meaningful.
inline int chain_shape(int32_t width, int32_t height, int32_t mipmapped, rtx_texture_desc * desc, int64_t * texel_count) {
    *desc = rtx_texture_desc();
    desc->width = width; desc->height = height;
    const bool pow2 = ((width & (width - 1)) == 0) && ((height & (height - 1)) == 0);      // Math::is_power_of_two, Texture.cpp:50
    desc->mipmapped = mipmapped && pow2 ? 1 : 0;
    desc->mip_levels = desc->mipmapped ? 1 + (int)log2f((float)(width < height ? width : height)) : 1;
    if (desc->mip_levels > RTX_MAX_MIP_LEVELS) return RTX_ERR_LIMIT;
    int64_t offset = 0;
    for (int l = 0; l < desc->mip_levels; l++) {
        if (offset > INT32_MAX) return RTX_ERR_LIMIT;
        desc->mip_offsets[l] = (int32_t)offset;
        offset += (int64_t)(width >> l) * (height >> l);
    }
    if (offset > INT32_MAX) return RTX_ERR_LIMIT;
    *texel_count = offset;
    return RTX_OK;
}

static_assert(BLOCK % TILE == 0 && PLANE_A >= 4 * PLANE_B, "tile_load takes a row per TILE threads; a halving fits the other buffer");

RTX_HD float box(float c0, float c1, float c2, float c3) { return (((c0 + c1) + c2) + c3) * 0.25f; }

struct Pass {
    int32_t src_level, src_w, src_h;            // the level the pass reads
    int32_t tiles_x, tiles_y;                   // its tile grid: one workgroup per tile
    int32_t levels;                             // levels made below the source, 0 .. MAX_PASS_LEVELS
    int32_t offset[MAX_PASS_LEVELS + 1];        // chain offsets (texels) of src_level .. src_level + levels
};
struct Plan { int32_t count; Pass pass[RTX_MAX_MIP_LEVELS]; };

// (width, height, levels) as chain_shape accepted them, P in 1 .. MAX_PASS_LEVELS
inline Plan plan_passes(int32_t width, int32_t height, int32_t levels, int32_t P) {
    int32_t offsets[RTX_MAX_MIP_LEVELS + 1] = { 0 };
    for (int l = 0; l < levels; l++) offsets[l + 1] = offsets[l] + (width >> l) * (height >> l);
    Plan plan; plan.count = 0;
    int s = 0;
    do {
        Pass & p = plan.pass[plan.count++];
        p = Pass();
        p.src_level = s; p.src_w = width >> s; p.src_h = height >> s;
        p.tiles_x = (p.src_w + TILE - 1) / TILE; p.tiles_y = (p.src_h + TILE - 1) / TILE;
        p.levels = levels - 1 - s < P ? levels - 1 - s : P;
        for (int k = 0; k <= p.levels; k++) p.offset[k] = offsets[s + k];
        s += p.levels;
    } while (s < levels - 1);
    return plan;
}

struct Tile { int32_t x0, y0, w, h; };          // in texels of the pass's source level
RTX_HD Tile pass_tile(const Pass & p, int32_t tile) {
    Tile t;
    t.x0 = (tile % p.tiles_x) * TILE; t.y0 = (tile / p.tiles_x) * TILE;
    t.w = p.src_w - t.x0 < TILE ? p.src_w - t.x0 : TILE;
    t.h = p.src_h - t.y0 < TILE ? p.src_h - t.y0 : TILE;
    return t;
}

// Thread tid of n: its texels of the tile from src (indexed by the texel's place in the source level) into the planes a[c * PLANE_A + y * t.w + x]
// and, with store, to dst as the pass's level 0.
template <typename Src, typename Dst> RTX_HD void tile_load(const Pass & p, const Tile & t, const Src & src, Dst & dst, bool store, float * a, int tid, int n) {
    const int x = (int)((unsigned)tid % TILE);              // a row of the tile per TILE threads (n is a multiple of TILE): no division by the tile's width
    if (x >= t.w) return;
    for (int y = (int)((unsigned)tid / TILE); y < t.h; y += n / TILE) {
        const int i = y * t.w + x;
        const int32_t at = (t.y0 + y) * p.src_w + t.x0 + x;
        float c[3];
        src.load(at, c);
        a[i] = c[0]; a[PLANE_A + i] = c[1]; a[2 * PLANE_A + i] = c[2];
        if (store) dst.store(p.offset[0] + at, c[0], c[1], c[2]);
    }
}

// Thread tid of n: its texels of the tile's halving number k (1 .. p.levels) from the planes `from` (stride from_plane, the tile at k - 1,
// rows of t.w >> (k - 1)) into the planes `to` (stride to_plane, rows of t.w >> k) and to dst at level src_level + k.
template <typename Dst> RTX_HD void tile_reduce(const Pass & p, const Tile & t, int k, const float * from, int from_plane, float * to, int to_plane, Dst & dst, int tid, int n) {
    const int fw = t.w >> (k - 1), w = t.w >> k, h = t.h >> k;
    const int32_t lw = p.src_w >> k, x0 = t.x0 >> k, y0 = t.y0 >> k;
    const int shift = __builtin_ctz((unsigned)w);            // a tile that is reduced is a power of two wide
    for (int o = tid; o < w * h; o += n) {
        const int i = o & (w - 1), j = o >> shift;
        const int f = 2 * j * fw + 2 * i;
        float c[3];
        for (int ch = 0; ch < 3; ch++) {
            const float * s = from + ch * from_plane + f;
            c[ch] = box(s[0], s[1], s[fw], s[fw + 1]);
            to[ch * to_plane + o] = c[ch];
        }
        dst.store(p.offset[k] + (y0 + j) * lw + x0 + i, c[0], c[1], c[2]);
    }
}

// The whole tile with the threads taken in turn (sync() = the workgroup barrier between two steps): the order of the steps and which of the
// two buffers a step reads and writes, for the kernel and the checker alike.  a: 3 * PLANE_A floats, b: 3 * PLANE_B floats.
template <typename Src, typename Dst, typename Threads, typename Sync>
RTX_HD void tile_run(const Pass & p, int32_t tile, const Src & src, Dst & dst, bool store, float * a, float * b, Threads && threads, Sync && sync) {
    const Tile t = pass_tile(p, tile);
    threads([&](int tid, int n) { tile_load(p, t, src, dst, store, a, tid, n); });
    for (int k = 1; k <= p.levels; k++) {
        sync();
        if (k & 1) threads([&](int tid, int n) { tile_reduce(p, t, k, a, PLANE_A, b, PLANE_B, dst, tid, n); });
        else       threads([&](int tid, int n) { tile_reduce(p, t, k, b, PLANE_B, a, PLANE_A, dst, tid, n); });
    }
}

}  // namespace rtxt
