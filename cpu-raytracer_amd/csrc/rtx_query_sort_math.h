// rtx_query_sort_math.h — the sort key of RTX_QUERY_SORT (include/rtx.h: rtx_query_closest / rtx_query_occluded), written once and compiled
// twice like rtx_update_math.h: by hipcc into the kernels of rtx_query.h and by the host compiler into rtxh_query_sort_order
// (host/rtx_host.cpp), the specification the device order is compared with, and into query_sort_check.cpp.  Both builds use unfused fp32
// (-ffp-contract=off) and a correctly rounded division; only + - * / and comparisons, no libm: every function here returns the same bits
// on the CPU and on gfx950.  Plain C++: no HIP types.
//
// The key of a row of one round (at most RTX_QUERY_CHUNK_RAYS rows, sorted on their own):
//   * a row is LIVE when the fill kernels trace it: a direction that is not (+-0, +-0, +-0), six finite origin / direction components and,
//     for a segment (7 floats), a maximum distance that is not a NaN.  Every other row is DEAD;
//   * six coordinates per live row: the origin, and c = direction / max(|d.x|, |d.y|, |d.z|), the direction's point on the unit cube (one
//     correctly rounded division per component; no normalisation, no rsqrt).  -0 is +0 in all six;
//   * per round the min and the max of each coordinate over the live rows (exact in fp32, so any reduction order gives them).  A coordinate
//     with max == min is degenerate and takes no key bits; with L coordinates left each takes b = min(16, 42 / L) bits;
//   * q = min((uint32)(t * (2^b - 1)), 2^b - 1), t = (x - min) / (max - min), truncated.  When max - min overflows fp32 (origins at +-3e38)
//     both differences are taken of the HALVED values instead, t = (x/2 - min/2) / (max/2 - min/2): halving is exact for such floats, the
//     quotient is the same real number, and nothing is infinite.  t is in [0, 1] either way; a t that is not >= 0 would be cell 0;
//   * a row of FOUR floats is a point with a maximum distance (rtx_query_nearest): live when x, y, z are finite and the maximum distance is
//     > 0 (csrc/rtx_nearest_math.h), coordinates 0..2 the point, 3..5 the constant +0: degenerate, so the point takes all the key bits;
//   * the Morton code takes the quantised coordinates bit by bit, most significant bit first, within a bit in the order o.x o.y o.z c.x c.y c.z;
//   * key = dead << 63 | code << 20 | row in round.  A total order: any correct sort gives one result; dead rows come last in row order.
#pragma once
#include <stdint.h>

#if !defined(RTX_HD)
#if defined(__HIPCC__)
#define RTX_HD __host__ __device__ inline
#else
#define RTX_HD inline
#endif
#endif

namespace rtxq {

enum { COORDS = 6, CODE_BITS = 42, MAX_COORD_BITS = 16, ROW_BITS = 20, KEY_BITS = 64, DEAD_BIT = 63 };
static_assert(CODE_BITS + ROW_BITS < DEAD_BIT, "the Morton code sits between the row and the dead flag");

RTX_HD uint32_t float_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
RTX_HD bool is_finite(float f) { return (float_bits(f) & 0x7f800000u) != 0x7f800000u; }
RTX_HD float canonical(float f) { return float_bits(f) == 0x80000000u ? 0.0f : f; }
RTX_HD float magnitude(float f) { return f < 0.0f ? -f : f; }

// a float as an unsigned integer of the same order, and back (rtx_update_math.h has the same pair; the bounds are min reductions over these)
RTX_HD uint32_t ordered_key(float f) { const uint32_t u = float_bits(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
RTX_HD float ordered_value(uint32_t k) { const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; __builtin_memcpy(&f, &u, 4); return f; }

// what k_query_fill / k_query_fill_segments trace (query_row_is_ray, and r[6] == r[6] for a segment)
RTX_HD bool row_is_live(const float * r, int row_floats) {
    if (row_floats == 4) return is_finite(r[0]) && is_finite(r[1]) && is_finite(r[2]) && r[3] > 0.0f;      // a point row
    bool finite = true;
    for (int k = 0; k < 6; k++) finite = finite && is_finite(r[k]);
    const bool zero = (r[3] == 0.0f) & (r[4] == 0.0f) & (r[5] == 0.0f);
    return finite && !zero && (row_floats < 7 || r[6] == r[6]);
}

// the six coordinates of a LIVE row
RTX_HD void coordinates(const float * r, float x[COORDS]) {
    const float ax = magnitude(r[3]), ay = magnitude(r[4]), az = magnitude(r[5]);
    float m = ax > ay ? ax : ay; m = m > az ? m : az;                  // > 0: the row is live
    for (int k = 0; k < 3; k++) { x[k] = canonical(r[k]); x[3 + k] = canonical(r[3 + k] / m); }
}

// ... of a live row of row_floats floats: a point row (4) has the point and three constant zeros
RTX_HD void coordinates(const float * r, int row_floats, float x[COORDS]) {
    if (row_floats == 4) { for (int k = 0; k < 3; k++) { x[k] = canonical(r[k]); x[3 + k] = 0.0f; } return; }
    coordinates(r, x);
}

// The twelve bounds of a round as the kernels reduce them: lo[0..5] as ordered keys, hi[0..5] as COMPLEMENTED ordered keys, so that both
// reduce by an unsigned min and one memset of 0xff initialises them.  A round without a live row keeps 0xffffffff everywhere.
RTX_HD void bounds_of_row(const float x[COORDS], uint32_t k12[2 * COORDS]) {
    for (int a = 0; a < COORDS; a++) { const uint32_t k = ordered_key(x[a]); k12[a] = k; k12[COORDS + a] = ~k; }
}

struct Plan {                       // the same for every row of a round
    int32_t live_coords;            // L: coordinates with max > min
    int32_t bits;                   // b: key bits per live coordinate (0 when L == 0)
    uint32_t used;                  // bit a: coordinate a is live
    float lo[COORDS], extent[COORDS], scale[COORDS];      // scale: 1, or 0.5 where max - min overflows (extent is then max/2 - min/2)
};

RTX_HD Plan make_plan(const uint32_t * bounds12) {
    Plan p;
    p.live_coords = 0; p.used = 0u;
    for (int a = 0; a < COORDS; a++) {
        p.lo[a] = 0.0f; p.extent[a] = 1.0f; p.scale[a] = 1.0f;
        const uint32_t klo = bounds12[a], khi = ~bounds12[COORDS + a];
        if (bounds12[a] == 0xffffffffu || !(khi > klo)) continue;    // no live row, or one value: degenerate
        const float lo = ordered_value(klo), hi = ordered_value(khi);
        float e = hi - lo, s = 1.0f;
        if (!is_finite(e)) { s = 0.5f; e = hi * 0.5f - lo * 0.5f; }
        p.lo[a] = lo; p.extent[a] = e; p.scale[a] = s;
        p.used |= 1u << a; p.live_coords++;
    }
    p.bits = p.live_coords == 0 ? 0 : (CODE_BITS / p.live_coords < MAX_COORD_BITS ? CODE_BITS / p.live_coords : MAX_COORD_BITS);
    return p;
}

// one live coordinate -> its cell, 0 .. 2^bits - 1
RTX_HD uint32_t quantise(const Plan & p, int a, float x) {
    const uint32_t top = (1u << p.bits) - 1u;
    const float t = (x * p.scale[a] - p.lo[a] * p.scale[a]) / p.extent[a];      // scale 1: x - lo, exactly
    if (!(t >= 0.0f)) return 0u;
    if (t >= 1.0f) return top;
    const uint32_t q = (uint32_t)(t * (float)top);
    return q > top ? top : q;
}

RTX_HD uint64_t morton(const Plan & p, const uint32_t q[COORDS]) {
    uint64_t code = 0;
    for (int k = p.bits - 1; k >= 0; k--)
        for (int a = 0; a < COORDS; a++) if ((p.used >> a) & 1u) code = (code << 1) | (uint64_t)((q[a] >> k) & 1u);
    return code;
}

// the key of row `row` (< 2^ROW_BITS) of a round
RTX_HD uint64_t sort_key(const Plan & p, const float * r, int row_floats, uint32_t row) {
    if (!row_is_live(r, row_floats)) return ((uint64_t)1 << DEAD_BIT) | (uint64_t)row;
    float x[COORDS]; uint32_t q[COORDS];
    coordinates(r, row_floats, x);
    for (int a = 0; a < COORDS; a++) q[a] = ((p.used >> a) & 1u) ? quantise(p, a, x[a]) : 0u;
    return (morton(p, q) << ROW_BITS) | (uint64_t)row;
}
RTX_HD uint32_t key_row(uint64_t key) { return (uint32_t)key & ((1u << ROW_BITS) - 1u); }
RTX_HD bool key_is_dead(uint64_t key) { return (key >> DEAD_BIT) != 0; }

}  // namespace rtxq
