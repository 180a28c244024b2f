// lone_check.cpp — the two scene facts of plan_lone_facts (rtx_plan.h) and the arithmetic rule the packet kernels' transform skip rests on, on
// the CPU: `make lone_check` builds this with -fsanitize=address,undefined and -ffp-contract=off and runs it.
//   * lone / copy_class on hand-made frames: the reference's two-slot TLAS of one instance, a second instance, a root that is an inner node, a
//     leaf of two, a slot that names another instance, no TLAS at all; matrices with +0 and -0 cells, a diagonal one ulp off 1, a 1e-45 cell,
//     a translation, and cells of the fourth row (which no transform reads);
//   * over 2^20 float32 vectors with +-0, subnormals, the largest finite values and seeded floats of every exponent mixed in, and every one of
//     the 512 sign patterns of the nine off-diagonal cells: xform_pos and xform_dir (restated from rtx_math.h:48-57, the same expressions in
//     the same order, nothing fused) return every non-zero component bit for bit and turn a zero component into a zero;
//   * the rule is not vacuous: zero components do change sign, under xform_pos and under xform_dir, which is why a packet with a zero
//     component takes the arithmetic.
// Needs no GPU and no ROCm.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "rtx_plan.h"

static int failures = 0;
static char current[128] = "";
#define CHECK(x) do { if (!(x)) { if (failures < 20) printf("FAILED [%s] line %d: %s\n", current, __LINE__, #x); failures++; } } while (0)

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static uint32_t rng_state = 11;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// rtx_math.h xform_pos / xform_dir, cells[i + 4j]: the expressions as written there
struct v3 { float x, y, z; };
static v3 xform_pos(const float * c, v3 d) {
    return v3{ c[0] * d.x + (c[1] * d.y + (c[2]  * d.z + c[3])),
               c[4] * d.x + (c[5] * d.y + (c[6]  * d.z + c[7])),
               c[8] * d.x + (c[9] * d.y + (c[10] * d.z + c[11])) };
}
static v3 xform_dir(const float * c, v3 d) {
    return v3{ c[0] * d.x + (c[1] * d.y + c[2]  * d.z),
               c[4] * d.x + (c[5] * d.y + c[6]  * d.z),
               c[8] * d.x + (c[9] * d.y + c[10] * d.z) };
}

// a finite float32: +-0, subnormals, the extremes, or any exponent
static float component() {
    static const uint32_t SPECIAL[] = { 0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u,
                                        0x7f7fffffu, 0xff7fffffu, 0x7f61b1e6u /* 3e38 */, 0xff61b1e6u, 0x3f800000u, 0xbf800000u };
    const uint32_t pick = rng() % 8u;
    if (pick < 2u) return from_bits(SPECIAL[rng() % (sizeof(SPECIAL) / sizeof(SPECIAL[0]))]);
    if (pick == 2u) return from_bits(((rng() & 1u) << 31) | (rng() & 0x7fffffu));                               // a subnormal (or a zero)
    return from_bits(((rng() & 1u) << 31) | ((1u + rng() % 254u) << 23) | (rng() & 0x7fffffu));                 // any normal exponent
}

static const int OFF_DIAGONAL[9] = { 1, 2, 3, 4, 6, 7, 8, 9, 11 };
// the matrix of the class whose off-diagonal cell k is -0 where bit k of `pattern` is set; the fourth row is garbage no transform reads
static void class_matrix(uint32_t pattern, float m[16]) {
    for (int k = 0; k < 16; k++) m[k] = k >= 12 ? 7.5f : 0.0f;
    m[0] = m[5] = m[10] = 1.0f;
    for (int k = 0; k < 9; k++) if ((pattern >> k) & 1u) m[OFF_DIAGONAL[k]] = -0.0f;
}

static LoneFacts facts(const std::vector<rtx_bvh_node> & nodes, const std::vector<int32_t> & idx, const std::vector<rtx_instance> & inst) {
    return plan_lone_facts((int)inst.size(), nodes.data(), (int)nodes.size(), idx.data(), (int)idx.size(), inst.data());
}

static rtx_bvh_node node(int32_t left_or_first, int32_t count) {
    rtx_bvh_node n; memset(&n, 0, sizeof(n));
    for (int a = 0; a < 3; a++) { n.aabb_min[a] = -1.0f; n.aabb_max[a] = 1.0f; }
    n.left_or_first = left_or_first; n.count = count;
    return n;
}

static rtx_instance instance(uint32_t pattern) {
    rtx_instance I; memset(&I, 0, sizeof(I));
    class_matrix(0u, I.world); class_matrix(pattern, I.world_inv);
    return I;
}

static void check_facts() {
    snprintf(current, sizeof(current), "facts");
    const rtx_bvh_node garbage = node(0x7fffffff, -5);                     // the unused slot 1 of a reference-built array
    {   // the reference's TLAS of one instance: a root leaf and the unused slot
        const LoneFacts f = facts({ node(0, 1), garbage }, { 0 }, { instance(0u) });
        CHECK(f.lone && f.copy_class);
        const LoneFacts g = facts({ node(0, 1) }, { 0 }, { instance(0x1ffu) });      // one slot only, every off-diagonal cell -0
        CHECK(g.lone && g.copy_class);
        const LoneFacts h = facts({ node(0, 1), garbage }, { 0 }, { instance(0x0a5u) });
        CHECK(h.lone && h.copy_class);
    }
    {   // not lone: a second instance (whatever the tree), an inner root, a leaf of two, a leaf with axis bits, a first slot other than 0,
        // a slot that names another instance, no TLAS, no indices
        CHECK(!facts({ node(0, 1), garbage }, { 0 }, { instance(0u), instance(0u) }).lone);
        CHECK(!facts({ node(2, 0), garbage, node(0, 1), node(1, 1) }, { 0, 1 }, { instance(0u), instance(0u) }).lone);
        CHECK(!facts({ node(2, 0), garbage, node(0, 1), node(0, 1) }, { 0 }, { instance(0u) }).lone);
        CHECK(!facts({ node(0, 2), garbage }, { 0, 0 }, { instance(0u) }).lone);
        CHECK(!facts({ node(0, 1 | (1 << 30)), garbage }, { 0 }, { instance(0u) }).lone);
        CHECK(!facts({ node(1, 1), garbage }, { 0, 0 }, { instance(0u) }).lone);
        CHECK(!facts({ node(0, 1), garbage }, { 1 }, { instance(0u) }).lone);
        CHECK(!facts({}, {}, { instance(0u) }).lone);
        CHECK(!facts({ node(0, 1) }, {}, { instance(0u) }).lone);
        CHECK(!facts({ node(0, 1) }, { 0 }, {}).lone);
        CHECK(!facts({ node(0, 1), garbage }, { 0 }, { instance(0u), instance(0u) }).copy_class);      // copy_class never without lone
    }
    {   // lone but not of the copy class: each of the twelve cells in turn one step away, and the usual moved instances
        for (int k = 0; k < 12; k++) {
            const bool diagonal = k == 0 || k == 5 || k == 10;
            const uint32_t wrong[] = { diagonal ? 0x3f800001u /* 1 + 2^-23 */ : 0x00000001u /* 1e-45 */, diagonal ? 0x3f7fffffu : 0x80000001u,
                                       diagonal ? 0xbf800000u /* -1 */ : 0x3f800000u, diagonal ? 0x00000000u : 0x7f800000u, 0x7fc00000u };
            for (uint32_t w : wrong) {
                rtx_instance I = instance(rng() & 0x1ffu);
                I.world_inv[k] = from_bits(w);
                const LoneFacts f = facts({ node(0, 1), garbage }, { 0 }, { I });
                CHECK(f.lone && !f.copy_class);
            }
        }
        rtx_instance moved = instance(0u); moved.world_inv[3] = -2.0f; moved.world[3] = 2.0f;
        CHECK(facts({ node(0, 1), garbage }, { 0 }, { moved }).lone && !facts({ node(0, 1), garbage }, { 0 }, { moved }).copy_class);
        rtx_instance turned = instance(0u); turned.world_inv[0] = 0.0f; turned.world_inv[2] = -1.0f; turned.world_inv[8] = 1.0f; turned.world_inv[10] = 0.0f;
        CHECK(facts({ node(0, 1), garbage }, { 0 }, { turned }).lone && !facts({ node(0, 1), garbage }, { 0 }, { turned }).copy_class);
    }
    {   // the fourth row and `world` are not read: any cells there
        rtx_instance I = instance(0x155u);
        for (int k = 12; k < 16; k++) I.world_inv[k] = from_bits(0x7fc00000u);
        for (int k = 0; k < 16; k++) I.world[k] = 3.0f;
        CHECK(facts({ node(0, 1), garbage }, { 0 }, { I }).copy_class);
    }
}

static long vectors = 0, zero_components = 0, flipped_pos = 0, flipped_dir = 0, nonzero_components = 0;

static void check_vector(const float m[16], v3 v) {
    const v3 p = xform_pos(m, v), d = xform_dir(m, v);
    const float in[3] = { v.x, v.y, v.z }, po[3] = { p.x, p.y, p.z }, dr[3] = { d.x, d.y, d.z };
    for (int a = 0; a < 3; a++) {
        if (in[a] != 0.0f) {
            nonzero_components++;
            CHECK(bits_of(po[a]) == bits_of(in[a]));
            CHECK(bits_of(dr[a]) == bits_of(in[a]));
        } else {
            zero_components++;
            CHECK((bits_of(po[a]) & 0x7fffffffu) == 0u);
            CHECK((bits_of(dr[a]) & 0x7fffffffu) == 0u);
            if (bits_of(po[a]) != bits_of(in[a])) flipped_pos++;
            if (bits_of(dr[a]) != bits_of(in[a])) flipped_dir++;
        }
    }
    vectors++;
}

static void check_arithmetic() {
    snprintf(current, sizeof(current), "arithmetic");
    float m[16];
    // every vector under all +0, all -0 and six more patterns; the patterns cycle, so each of the 512 meets 2^14 vectors
    const long N = 1l << 20;
    for (long i = 0; i < N; i++) {
        const v3 v = { component(), component(), component() };
        class_matrix(0u, m); check_vector(m, v);
        class_matrix(0x1ffu, m); check_vector(m, v);
        for (int k = 0; k < 6; k++) { class_matrix((uint32_t)((i * 6 + k) & 0x1ff), m); check_vector(m, v); }
    }
    // and every pattern over the corner cases: each component each special value
    const uint32_t corner[] = { 0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x7f7fffffu, 0xff7fffffu, 0x3f800000u, 0xc0490fdbu };
    for (uint32_t pattern = 0; pattern < 512u; pattern++) {
        class_matrix(pattern, m);
        for (uint32_t x : corner) for (uint32_t y : corner) for (uint32_t z : corner) check_vector(m, v3{ from_bits(x), from_bits(y), from_bits(z) });
    }
    CHECK(vectors >= 8 * N);
    CHECK(zero_components > N / 8 && nonzero_components > N);
    CHECK(flipped_pos > zero_components / 20 && flipped_dir > zero_components / 20);      // not vacuous: the sign of a zero does move
}

int main() {
    check_facts();
    check_arithmetic();
    printf("lone_check: %ld vector transforms, %ld non-zero components copied, %ld zero components, sign changed under xform_pos %ld (%.1f %%), under xform_dir %ld (%.1f %%)\n",
           vectors, nonzero_components, zero_components, flipped_pos, 100.0 * (double)flipped_pos / (double)zero_components, flipped_dir,
           100.0 * (double)flipped_dir / (double)zero_components);
    if (failures) { printf("lone_check: %d FAILED\n", failures); return 1; }
    printf("lone_check: ok\n");
    return 0;
}
