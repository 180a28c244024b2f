// texmip_check.cpp — the pass plan of rtx_update_texture (rtx_texmip_math.h) on the CPU: `make texmip_check` builds this with
// -fsanitize=address,undefined and runs it.  For every shape the GPU tests use and every P in 1 .. 5 it runs each pass and each tile through
// rtxt::tile_run — the code k_texmip runs, with a loop over the 256 threads where the kernel has its lanes and nothing where it has its
// barrier — into a chain that counts its stores, and compares the result bit for bit (NaN equal to NaN) with the plain loop, level by level,
// of Texture::load (Texture.cpp:76-117).  Checked on the way: every texel of every level is stored exactly once, every tile lies inside
// its level, no load leaves the source level.  Needs no GPU and no ROCm.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "rtx_texmip_math.h"

static int failures = 0;
static char current[128] = "";
#define CHECK(x) do { if (!(x)) { if (failures < 20) printf("FAILED [%s] line %d: %s\n", current, __LINE__, #x); failures++; } } while (0)

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }

static uint32_t rng_state = 1;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// seeded floats over many exponents and both signs, and a block of subnormals, near-FLT_MAX values whose sums overflow, infinities, NaNs, -0.0
static std::vector<float> level0(int w, int h) {
    std::vector<float> t((size_t)w * h * 3);
    for (float & v : t) v = from_bits(((rng() & 1u) << 31) | ((90u + rng() % 70u) << 23) | (rng() & 0x7fffffu));
    const uint32_t planted[] = { 0x00000001u, 0x807fffffu, 0x00400000u, 0x7f7fffffu, 0x7f7ffff0u, 0xff7fffffu, 0x7f000000u, 0x7f800000u, 0xff800000u,
                                 0x7fc00000u, 0xffc00001u, 0x7f800001u, 0x80000000u, 0x00000000u };
    const size_t n = sizeof(planted) / sizeof(planted[0]);
    for (size_t i = 0; i < t.size() && i < 4 * n * 3; i++) t[i] = from_bits(planted[(i * 7 + i / n) % n]);
    return t;
}

struct SrcRgb   { const float * p; int64_t count; void load(int32_t at, float c[3]) const { CHECK(at >= 0 && at < count); if (at < 0 || at >= count) { c[0] = c[1] = c[2] = 0; return; } memcpy(c, p + 3 * (size_t)at, 12); } };
struct Quad4    { float x, y, z, w; };
struct SrcChain { const Quad4 * p; int64_t count; void load(int32_t at, float c[3]) const { CHECK(at >= 0 && at < count); if (at < 0 || at >= count) { c[0] = c[1] = c[2] = 0; return; } c[0] = p[at].x; c[1] = p[at].y; c[2] = p[at].z; } };
struct DstChain {
    std::vector<Quad4> texels; std::vector<int> stores;
    void store(int32_t at, float r, float g, float b) {
        CHECK(at >= 0 && (size_t)at < texels.size());
        if (at < 0 || (size_t)at >= texels.size()) return;
        texels[at] = Quad4{ r, g, b, 0.0f }; stores[at]++;
    }
};

static void run_shape(int w, int h, int mipmapped, int P) {
    snprintf(current, sizeof(current), "%d x %d mipmapped %d P %d", w, h, mipmapped, P);
    rtx_texture_desc d; int64_t count = 0;
    CHECK(rtxt::chain_shape(w, h, mipmapped, &d, &count) == RTX_OK);
    const bool pow2 = !(w & (w - 1)) && !(h & (h - 1));
    int want_levels = 1;
    if (mipmapped && pow2) for (int m = (w < h ? w : h); m > 1; m >>= 1) want_levels++;
    CHECK(d.width == w && d.height == h && d.mip_levels == want_levels && d.mipmapped == (mipmapped && pow2 ? 1 : 0));
    const std::vector<float> src = level0(w, h);

    // the plain loop: level 0 as given, every further level from the stored texels of the one before
    std::vector<float> want((size_t)count * 3);
    memcpy(want.data(), src.data(), src.size() * 4);
    int64_t at = 0;
    for (int l = 0; l < d.mip_levels; l++) {
        CHECK(d.mip_offsets[l] == at);
        at += (int64_t)(w >> l) * (h >> l);
        if (l == 0) continue;
        const int lw = w >> l, lh = h >> l, pw = w >> (l - 1);
        for (int j = 0; j < lh; j++) for (int i = 0; i < lw; i++) for (int k = 0; k < 3; k++) {
            const float * p = want.data() + 3 * (size_t)d.mip_offsets[l - 1] + k;
            want[3 * ((size_t)d.mip_offsets[l] + i + (size_t)j * lw) + k] =
                rtxt::box(p[3 * ((size_t)2 * i + (size_t)2 * j * pw)], p[3 * ((size_t)2 * i + 1 + (size_t)2 * j * pw)],
                          p[3 * ((size_t)2 * i + (size_t)(2 * j + 1) * pw)], p[3 * ((size_t)2 * i + 1 + (size_t)(2 * j + 1) * pw)]);
        }
    }
    CHECK(at == count);

    // the pass plan, as rtx_update_texture launches it
    const rtxt::Plan plan = rtxt::plan_passes(w, h, d.mip_levels, P);
    DstChain dst; dst.texels.assign((size_t)count, Quad4{ -1.0f, -1.0f, -1.0f, -1.0f }); dst.stores.assign((size_t)count, 0);
    std::vector<float> a(3 * rtxt::PLANE_A), b(3 * rtxt::PLANE_B);       // exactly the kernel's LDS: a read or write past them is the sanitizer's
    const auto threads = [](auto && body) { for (int tid = 0; tid < rtxt::BLOCK; tid++) body(tid, (int)rtxt::BLOCK); };
    const auto sync = [] {};
    int next_src = 0;
    CHECK(plan.count >= 1 && plan.count <= RTX_MAX_MIP_LEVELS);
    for (int k = 0; k < plan.count; k++) {
        const rtxt::Pass & p = plan.pass[k];
        CHECK(p.src_level == next_src && p.src_w == (w >> p.src_level) && p.src_h == (h >> p.src_level));
        CHECK(p.levels >= (d.mip_levels > 1 ? 1 : 0) && p.levels <= P && p.src_level + p.levels < d.mip_levels);
        CHECK(p.tiles_x * rtxt::TILE >= p.src_w && (p.tiles_x - 1) * rtxt::TILE < p.src_w && p.tiles_y * rtxt::TILE >= p.src_h && (p.tiles_y - 1) * rtxt::TILE < p.src_h);
        for (int l = 0; l <= p.levels; l++) CHECK(p.offset[l] == d.mip_offsets[p.src_level + l]);
        next_src = p.src_level + p.levels;
        for (int t = 0; t < p.tiles_x * p.tiles_y; t++) {
            const rtxt::Tile T = rtxt::pass_tile(p, t);
            CHECK(T.x0 >= 0 && T.y0 >= 0 && T.w >= 1 && T.h >= 1 && T.w <= rtxt::TILE && T.h <= rtxt::TILE && T.x0 + T.w <= p.src_w && T.y0 + T.h <= p.src_h);
            CHECK(p.levels == 0 || ((T.w >> p.levels) >= 1 && (T.h >> p.levels) >= 1 && T.x0 % rtxt::TILE == 0 && T.y0 % rtxt::TILE == 0 && !(T.w & (T.w - 1)) && !(T.h & (T.h - 1))));
            if (k == 0) { const SrcRgb s = { src.data(), (int64_t)w * h }; rtxt::tile_run(p, t, s, dst, true, a.data(), b.data(), threads, sync); }
            else { const SrcChain s = { dst.texels.data() + p.offset[0], (int64_t)p.src_w * p.src_h }; rtxt::tile_run(p, t, s, dst, false, a.data(), b.data(), threads, sync); }
        }
    }
    CHECK(next_src == d.mip_levels - 1);
    size_t wrong = 0, not_once = 0;
    for (size_t i = 0; i < (size_t)count; i++) {
        if (dst.stores[i] != 1) not_once++;
        if (!same(dst.texels[i].x, want[3 * i]) || !same(dst.texels[i].y, want[3 * i + 1]) || !same(dst.texels[i].z, want[3 * i + 2]) || bits(dst.texels[i].w) != 0u) wrong++;
    }
    CHECK(not_once == 0);
    CHECK(wrong == 0);
}

int main() {
    static const int shapes[][3] = { { 1, 1, 1 }, { 2, 1, 1 }, { 1, 2, 1 }, { 2, 2, 1 }, { 4, 4, 1 }, { 32, 32, 1 }, { 64, 64, 1 }, { 64, 32, 1 }, { 32, 64, 1 }, { 128, 2, 1 },
                                     { 2, 128, 1 }, { 256, 256, 1 }, { 2048, 64, 1 }, { 33, 31, 1 }, { 3, 5, 1 }, { 300, 200, 1 }, { 64, 64, 0 }, { 64, 16, 1 } };
    for (int P = 1; P <= rtxt::MAX_PASS_LEVELS; P++) for (const auto & s : shapes) run_shape(s[0], s[1], s[2], P);
    run_shape(2048, 2048, 1, 5);

    snprintf(current, sizeof(current), "plans and limits");
    CHECK(rtxt::plan_passes(2048, 2048, 12, 5).count == 3 && rtxt::plan_passes(2048, 2048, 12, 1).count == 11);
    CHECK(rtxt::plan_passes(256, 256, 9, rtxt::DEFAULT_PASS_LEVELS).count == 2);      // the default: five levels per launch
    CHECK(rtxt::plan_passes(256, 256, 9, 5).count == 2 && rtxt::plan_passes(256, 256, 9, 5).pass[1].src_level == 5);
    { const rtxt::Plan p = rtxt::plan_passes(2048, 64, 7, 5); CHECK(p.count == 2 && p.pass[1].src_w == 64 && p.pass[1].src_h == 2 && p.pass[1].levels == 1 && p.pass[1].tiles_x == 2 && p.pass[1].tiles_y == 1); }
    CHECK(rtxt::plan_passes(300, 200, 1, 5).count == 1 && rtxt::plan_passes(300, 200, 1, 5).pass[0].levels == 0 && rtxt::plan_passes(300, 200, 1, 5).pass[0].tiles_x == 10);
    rtx_texture_desc d; int64_t n = 0;
    CHECK(rtxt::chain_shape(32768, 32768, 1, &d, &n) == RTX_OK && d.mip_levels == 16 && n == 1431655765);
    CHECK(rtxt::chain_shape(65536, 65536, 1, &d, &n) == RTX_ERR_LIMIT);          // 17 levels
    CHECK(rtxt::chain_shape(65536, 32768, 0, &d, &n) == RTX_ERR_LIMIT);          // 2^31 texels
    CHECK(rtxt::chain_shape(46341, 46341, 1, &d, &n) == RTX_ERR_LIMIT && rtxt::chain_shape(46340, 46340, 1, &d, &n) == RTX_OK && n == 2147395600);
    CHECK(bits(rtxt::box(from_bits(1u), 0.0f, 0.0f, 0.0f)) == 0u && bits(rtxt::box(from_bits(4u), 0.0f, 0.0f, 0.0f)) == 1u);      // subnormals are not flushed
    CHECK(bits(rtxt::box(3e38f, 3e38f, -3e38f, -3e38f)) == 0x7f800000u);                                                           // the sum overflows where it does in the reference's order

    if (failures) { printf("texmip_check: %d FAILED\n", failures); return 1; }
    printf("texmip_check: ok\n");
    return 0;
}
