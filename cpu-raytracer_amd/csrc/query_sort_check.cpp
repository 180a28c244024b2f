// query_sort_check.cpp — the sort key of RTX_QUERY_SORT (rtx_query_sort_math.h) on the CPU: `make query_sort_check` builds this with
// -fsanitize=address,undefined and runs it.  Rows are drawn from a pool of hostile floats (NaNs, infinities, -0, subnormals, +-FLT_MAX,
// +-3e38) and from seeded floats of many exponents; for row widths 6 and 7 and round sizes around a packet it checks that
//   * every row gets a key (no conversion out of range, no shift beyond its type: the sanitizer's part) and the key's layout holds: bit 63
//     the dead flag, bit 62 clear, the Morton code in L * b <= 42 bits above bit 20, the row below; a dead row's code is 0;
//   * live is what the fill kernels trace, and the quantised cells are below 2^b with the minimum in cell 0 and the maximum in the top cell;
//   * the bounds are the same for any reduction order, and -0 and +0 rows get equal codes;
//   * the sorted keys are a permutation of the rows with the dead rows last in row order, and equal live rows keep their row order.
// Needs no GPU and no ROCm.
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "rtx_query_sort_math.h"

static int failures = 0;
static char current[128] = "";
#define CHECK(x) do { if (!(x)) { if (failures < 20) printf("FAILED [%s] line %d: %s\n", current, __LINE__, #x); failures++; } } while (0)

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static uint32_t rng_state = 7;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static const uint32_t HOSTILE[] = { 0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x7f7fffffu, 0xff7fffffu,
                                    0x7f61b1e6u /* 3e38 */, 0xff61b1e6u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00001u, 0x7f800001u, 0x3f800000u, 0xbf800000u };
static float hostile() { return from_bits(HOSTILE[rng() % (sizeof(HOSTILE) / sizeof(HOSTILE[0]))]); }
static float seeded() { return from_bits(((rng() & 1u) << 31) | ((100u + rng() % 56u) << 23) | (rng() & 0x7fffffu)); }

// mix: 0 seeded floats only, 1 one hostile component in a few rows, 2 hostile components everywhere
static std::vector<float> make_rows(int m, int row_floats, int mix) {
    std::vector<float> r((size_t)m * row_floats);
    for (float & v : r) v = seeded();
    if (mix == 1) for (int i = 0; i < m; i += 3) r[(size_t)i * row_floats + rng() % row_floats] = hostile();
    if (mix == 2) for (float & v : r) if (rng() % 3) v = hostile();
    return r;
}

static void reduce_bounds(const std::vector<float> & rows, int m, int row_floats, bool backwards, uint32_t bounds[12]) {
    for (int a = 0; a < 12; a++) bounds[a] = 0xffffffffu;
    for (int s = 0; s < m; s++) {
        const int i = backwards ? m - 1 - s : s;
        const float * r = rows.data() + (size_t)i * row_floats;
        if (!rtxq::row_is_live(r, row_floats)) continue;
        float x[6]; uint32_t k12[12];
        rtxq::coordinates(r, x);
        for (int a = 0; a < 6; a++) CHECK(x[a] == x[a] && rtxq::is_finite(x[a]) && rtxq::float_bits(x[a]) != 0x80000000u);
        for (int a = 3; a < 6; a++) CHECK(x[a] >= -1.0f && x[a] <= 1.0f);
        rtxq::bounds_of_row(x, k12);
        for (int a = 0; a < 12; a++) if (k12[a] < bounds[a]) bounds[a] = k12[a];
    }
}

static bool live_by_hand(const float * r, int row_floats) {
    for (int k = 0; k < 6; k++) if (r[k] != r[k] || r[k] - r[k] != 0.0f) return false;      // NaN or infinite
    if (r[3] == 0.0f && r[4] == 0.0f && r[5] == 0.0f) return false;
    return row_floats < 7 || r[6] == r[6];
}

static void run(int m, int row_floats, int mix, std::vector<float> rows) {
    snprintf(current, sizeof(current), "m %d width %d mix %d", m, row_floats, mix);
    uint32_t bounds[12], back[12];
    reduce_bounds(rows, m, row_floats, false, bounds);
    reduce_bounds(rows, m, row_floats, true, back);
    CHECK(memcmp(bounds, back, sizeof(bounds)) == 0);
    const rtxq::Plan p = rtxq::make_plan(bounds);
    CHECK(p.live_coords >= 0 && p.live_coords <= 6 && p.bits >= 0 && p.bits <= 16 && p.live_coords * p.bits <= 42);
    CHECK(p.live_coords == 0 || p.bits == (42 / p.live_coords < 16 ? 42 / p.live_coords : 16));
    for (int a = 0; a < 6; a++) CHECK(p.extent[a] > 0.0f && rtxq::is_finite(p.extent[a]) && rtxq::is_finite(p.lo[a]));
    std::vector<uint64_t> keys((size_t)m);
    int dead = 0;
    bool seen_lo[6] = { false, false, false, false, false, false }, seen_hi[6] = { false, false, false, false, false, false };
    for (int i = 0; i < m; i++) {
        const float * r = rows.data() + (size_t)i * row_floats;
        const uint64_t k = rtxq::sort_key(p, r, row_floats, (uint32_t)i);
        keys[i] = k;
        const bool live = rtxq::row_is_live(r, row_floats);
        CHECK(live == live_by_hand(r, row_floats));
        CHECK(rtxq::key_row(k) == (uint32_t)i);
        CHECK(rtxq::key_is_dead(k) == !live);
        CHECK(((k >> 62) & 1) == 0);
        const uint64_t code = (k >> 20) & (((uint64_t)1 << 42) - 1);
        CHECK(code >> (p.live_coords * p.bits) == 0);
        if (!live) { dead++; CHECK(code == 0); continue; }
        float x[6];
        rtxq::coordinates(r, x);
        for (int a = 0; a < 6; a++) if ((p.used >> a) & 1u) {
            const uint32_t q = rtxq::quantise(p, a, x[a]), top = (1u << p.bits) - 1u;
            CHECK(q <= top);
            if (rtxq::ordered_key(x[a]) == bounds[a]) { CHECK(q == 0); seen_lo[a] = true; }
            if (rtxq::ordered_key(x[a]) == ~bounds[6 + a]) { CHECK(q == top); seen_hi[a] = true; }
        }
        // the same row with every zero's sign flipped: the same code
        float z[7];
        for (int c = 0; c < row_floats; c++) z[c] = r[c] == 0.0f ? -r[c] : r[c];
        CHECK(rtxq::sort_key(p, z, row_floats, (uint32_t)i) == k);
    }
    for (int a = 0; a < 6; a++) if ((p.used >> a) & 1u) CHECK(seen_lo[a] && seen_hi[a]);
    std::vector<uint64_t> sorted(keys);
    std::sort(sorted.begin(), sorted.end());
    std::vector<int> count((size_t)m, 0);
    for (int i = 0; i < m; i++) { const uint32_t row = rtxq::key_row(sorted[i]); CHECK(row < (uint32_t)m); if (row < (uint32_t)m) count[row]++; }
    for (int i = 0; i < m; i++) CHECK(count[i] == 1);
    for (int i = 0; i < m; i++) CHECK(rtxq::key_is_dead(sorted[i]) == (i >= m - dead));
    for (int i = m - dead + 1; i < m; i++) CHECK(rtxq::key_row(sorted[i - 1]) < rtxq::key_row(sorted[i]));
}

int main() {
    for (int row_floats = 6; row_floats <= 7; row_floats++)
        for (int mix = 0; mix <= 2; mix++)
            for (int m : { 1, 2, 63, 64, 65, 257, 4097 }) run(m, row_floats, mix, make_rows(m, row_floats, mix));
    for (int row_floats = 6; row_floats <= 7; row_floats++) {
        // origins at +-3e38 and +-FLT_MAX on every axis: the extent overflows, the keys do not
        std::vector<float> rows = make_rows(64, row_floats, 0);
        for (int i = 0; i < 64; i++) for (int a = 0; a < 3; a++) rows[(size_t)i * row_floats + a] = from_bits(HOSTILE[7 + (i + a) % 4]);
        for (int a = 0; a < 3; a++) rows[(size_t)5 * row_floats + a] = 0.0f;
        run(64, row_floats, 3, rows);
        // all live rows equal: no live coordinate, code 0, the order is the row order
        for (int i = 0; i < 64; i++) for (int c = 0; c < row_floats; c++) rows[(size_t)i * row_floats + c] = rows[c];
        run(64, row_floats, 4, rows);
        uint32_t bounds[12];
        reduce_bounds(rows, 64, row_floats, false, bounds);
        snprintf(current, sizeof(current), "equal rows width %d", row_floats);
        CHECK(rtxq::make_plan(bounds).live_coords == 0 && rtxq::make_plan(bounds).bits == 0);
        // no live row at all
        for (int i = 0; i < 64; i++) for (int c = 3; c < 6; c++) rows[(size_t)i * row_floats + c] = (i & 1) ? 0.0f : -0.0f;
        run(64, row_floats, 5, rows);
        // subnormal directions: the cube point is still inside the cube
        rows = make_rows(64, row_floats, 0);
        for (int i = 0; i < 64; i++) for (int a = 3; a < 6; a++) rows[(size_t)i * row_floats + a] = from_bits(((rng() & 1u) << 31) | (rng() & 0x7fffffu));
        run(64, row_floats, 6, rows);
    }
    if (failures) { printf("query_sort_check: %d FAILED\n", failures); return 1; }
    printf("query_sort_check: ok\n");
    return 0;
}
