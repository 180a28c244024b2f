// side_check.cpp — the device plan of rtx_blas_pseudonormals run on the CPU through the functions the kernels call (rtx_side_math.h, over the
// inverted index of rtx_normals_math.h): keys, a sort, the lower-bound offsets, the face records, the list walk per vertex and per slot
// edge — compared bit for bit with the plain loop rtxh_blas_pseudonormals is written as.  Shapes: one triangle, fans of valence 65 and 257, a
// boundary edge, a non-manifold edge of three faces, pad triangles and pad slots, repeated slots, the golden meshes, hostile floats.  No table
// component is ever NaN or infinite.  And the region: triangle_region is the branch triangle_d2 took — against a restated chain, with the
// (u, v) of triangle_d2 bit for bit, on every Voronoi border of the test triangles.  Built with the host sanitizers (make side_check): no GPU,
// no ROCm.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <limits>
#include <string>
#include <vector>
#include "rtx_side_math.h"

struct Rec4 { float x, y, z, w; };                      // the float4 of the device
struct Mesh {
    std::string name; std::vector<float> pos; std::vector<int32_t> idx, slots;      // slots: slot -> vertex table, 3 per slot
    int32_t T() const { return (int32_t)(idx.size() / 3); } int32_t V() const { return (int32_t)(pos.size() / 3); } int32_t S() const { return (int32_t)(slots.size() / 3); }
};

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("side_check: FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint32_t rng_state = 24680u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf() { return (float)rnd() / 16777216.0f * 2.0f - 1.0f; }

struct Tables { std::vector<float> vert, edge; };

// the host twin's loop: records, then over triangles and corners acc[v] += corner vector; the lists an edge walks filled by counting
static Tables plain_loop(const Mesh & m) {
    const int32_t T = m.T(), V = m.V(), S = m.S();
    Tables out; out.vert.assign((size_t)4 * V, 0.0f); out.edge.assign((size_t)12 * S, 0.0f);
    std::vector<float> rec((size_t)16 * T), acc((size_t)3 * V, 0.0f);
    for (int32_t t = 0; t < T; t++) rtxsd::triangle_record(m.idx.data(), m.pos.data(), (uint32_t)t, V, &rec[16 * (size_t)t]);
    for (int32_t t = 0; t < T; t++) {
        const int32_t * const tri = &m.idx[3 * (size_t)t];
        if (!rtxn::valid_triangle(tri[0], tri[1], tri[2], V)) continue;
        for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) acc[3 * (size_t)tri[k] + a] += rec[16 * (size_t)t + 4 + 4 * k + a];
    }
    for (int32_t v = 0; v < V; v++) rtxsd::finish_sum(&acc[3 * (size_t)v], &out.vert[4 * (size_t)v]);
    for (int32_t e = 0; e < 3 * S; e++) {
        int32_t x, y;
        rtxsd::edge_vertices(&m.slots[3 * (size_t)(e / 3)], e % 3, x, y);
        float s[3] = { 0.0f, 0.0f, 0.0f };
        if (x >= 0 && x < V && y >= 0 && y < V)
            for (int32_t t = 0; t < T; t++) {
                const int32_t * const tri = &m.idx[3 * (size_t)t];
                if (!rtxn::valid_triangle(tri[0], tri[1], tri[2], V)) continue;
                for (int k = 0; k < 3; k++) if (tri[k] == x && rtxsd::has_vertex(tri, y)) for (int a = 0; a < 3; a++) s[a] += rec[16 * (size_t)t + a];
            }
        rtxsd::finish_sum(s, &out.edge[4 * (size_t)e]);
    }
    return out;
}

// the device plan, launch by launch
static Tables device_plan(const Mesh & m) {
    const int32_t T = m.T(), V = m.V(), S = m.S();
    const uint32_t n = 3u * (uint32_t)T;
    std::vector<int32_t> indices(n); std::vector<uint64_t> keys(n);
    for (uint32_t c = 0; c < n; c++) {                  // k_normals_keys
        const uint32_t t = c / 3u;
        const int32_t tri[3] = { m.idx[3 * (size_t)t], m.idx[3 * (size_t)t + 1], m.idx[3 * (size_t)t + 2] };
        indices[c] = tri[c - 3u * t];
        keys[c] = rtxn::corner_key(tri, c, V);
    }
    std::reverse(keys.begin(), keys.end());
    std::sort(keys.begin(), keys.end());                // the radix sort
    std::vector<uint32_t> offset((size_t)V + 1);        // k_normals_offsets
    for (uint32_t v = 0; v <= (uint32_t)V; v++) offset[v] = rtxn::lower_bound(keys.data(), n, (uint64_t)v << 32);
    std::vector<Rec4> record((size_t)RTX_SIDE_RECORD * T);      // k_side_faces
    for (int32_t t = 0; t < T; t++) {
        float rec[16];
        rtxsd::triangle_record(indices.data(), m.pos.data(), (uint32_t)t, V, rec);
        for (int q = 0; q < 4; q++) record[RTX_SIDE_RECORD * (size_t)t + q] = Rec4{ rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3] };
    }
    Tables out; out.vert.assign((size_t)4 * V, 0.0f); out.edge.assign((size_t)12 * S, 0.0f);
    for (int32_t v = 0; v < V; v++) rtxsd::vertex_pseudonormal(keys.data(), offset[v], offset[v + 1], record.data(), &out.vert[4 * (size_t)v]);      // k_side_vertices
    for (int32_t e = 0; e < 3 * S; e++) {               // k_side_edges
        const int32_t s = e / 3;
        const int32_t sv[3] = { m.slots[3 * (size_t)s], m.slots[3 * (size_t)s + 1], m.slots[3 * (size_t)s + 2] };
        int32_t x, y;
        rtxsd::edge_vertices(sv, e - 3 * s, x, y);
        rtxsd::edge_pseudonormal(keys.data(), offset.data(), indices.data(), record.data(), V, x, y, &out.edge[4 * (size_t)e]);
    }
    return out;
}

static bool same_bits(const float * a, const float * b, size_t n) { return memcmp(a, b, n * 4) == 0; }
static bool all_zero_bits(const float * a, size_t n) { for (size_t k = 0; k < n; k++) { uint32_t u; memcpy(&u, a + k, 4); if (u) return false; } return true; }

static Tables run(const Mesh & m) {
    CHECK(m.T() >= 1 && m.V() >= 1, "%s: empty", m.name.c_str());
    const Tables a = plain_loop(m), b = device_plan(m);
    CHECK(a.vert.size() == b.vert.size() && same_bits(a.vert.data(), b.vert.data(), a.vert.size()), "%s: vertex tables of the device plan and the plain loop differ", m.name.c_str());
    CHECK(a.edge.size() == b.edge.size() && same_bits(a.edge.data(), b.edge.data(), a.edge.size()), "%s: edge tables of the device plan and the plain loop differ", m.name.c_str());
    for (size_t k = 0; k < a.vert.size(); k++) CHECK(rtxu::is_finite(a.vert[k]), "%s: vertex table component %zu is not finite", m.name.c_str(), k);
    for (size_t k = 0; k < a.edge.size(); k++) CHECK(rtxu::is_finite(a.edge[k]), "%s: edge table component %zu is not finite", m.name.c_str(), k);
    return a;
}

// ---- the shapes ----------------------------------------------------------------------------------------------------------------------------
static void identity_slots(Mesh & m) { m.slots = m.idx; }
static Mesh soup(const char * name, int32_t T, int32_t V) {
    Mesh m; m.name = name;
    for (int32_t k = 0; k < 3 * V; k++) m.pos.push_back(rndf());
    for (int32_t k = 0; k < 3 * T; k++) m.idx.push_back((int32_t)(rnd() % (uint32_t)V));
    identity_slots(m);
    return m;
}
static Mesh fan(const char * name, int32_t valence) {
    Mesh m; m.name = name;
    m.pos = { 0.0f, 0.3f, 0.0f };
    for (int32_t k = 0; k < valence; k++) { const float a = 6.2831853f * (float)k / (float)valence; m.pos.push_back(cosf(a)); m.pos.push_back(0.05f * rndf()); m.pos.push_back(sinf(a)); }
    for (int32_t k = 0; k < valence; k++) { m.idx.push_back(0); m.idx.push_back(1 + (k + 1) % valence); m.idx.push_back(1 + k); }
    identity_slots(m);
    return m;
}
static Mesh grid(const char * name, int32_t rows, int32_t cols) {
    Mesh m; m.name = name;
    for (int32_t i = 0; i < rows; i++) for (int32_t j = 0; j < cols; j++) {
        const float a = 6.2831853f * (float)i / (float)rows, b = 6.2831853f * (float)j / (float)cols;
        m.pos.push_back((2.0f + 0.7f * cosf(b)) * cosf(a)); m.pos.push_back(0.7f * sinf(b)); m.pos.push_back((2.0f + 0.7f * cosf(b)) * sinf(a));
    }
    for (int32_t i = 0; i < rows; i++) for (int32_t j = 0; j < cols; j++) {
        const int32_t a = i * cols + j, b = i * cols + (j + 1) % cols, c = ((i + 1) % rows) * cols + j, d = ((i + 1) % rows) * cols + (j + 1) % cols;
        m.idx.insert(m.idx.end(), { a, c, b, b, c, d });
    }
    identity_slots(m);
    return m;
}
static bool load_obj(const std::string & path, Mesh & m) {
    FILE * f = fopen(path.c_str(), "r");
    if (!f) return false;
    char line[512];
    while (fgets(line, sizeof(line), f)) {
        if (line[0] == 'v' && line[1] == ' ') { float x, y, z; if (sscanf(line + 2, "%f %f %f", &x, &y, &z) == 3) { m.pos.push_back(x); m.pos.push_back(y); m.pos.push_back(z); } }
        else if (line[0] == 'f' && line[1] == ' ') {
            std::vector<int32_t> poly;
            for (char * tok = strtok(line + 2, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) poly.push_back((int32_t)atoi(tok) - 1);
            for (size_t k = 2; k < poly.size(); k++) { m.idx.push_back(poly[0]); m.idx.push_back(poly[k - 1]); m.idx.push_back(poly[k]); }
        }
    }
    fclose(f);
    identity_slots(m);
    return !m.pos.empty() && !m.idx.empty();
}

// ---- the region -------------------------------------------------------------------------------------------------------------------------
// TRIANGLE of rtx_nearest_math.h restated: which branch applies
static int restated_region(rtxnp::P3 ap, rtxnp::P3 e1, rtxnp::P3 e2) {
    using rtxnp::dot;
    const float d1 = dot(e1, ap), d2 = dot(e2, ap), aa = dot(e1, e1), ab = dot(e1, e2), cc = dot(e2, e2);
    const float d3 = d1 - aa, d4 = d2 - ab, d5 = d1 - ab, d6 = d2 - cc;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0f && d2 <= 0.0f) return 0;
    if (d3 >= 0.0f && d4 <= d3) return 1;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) return 3;
    if (d6 >= 0.0f && d5 <= d6) return 2;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) return 5;
    if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) return 4;
    return 6;
}
static int region_points = 0, region_seen[7] = { 0, 0, 0, 0, 0, 0, 0 };
static void region_point(rtxnp::P3 ap, rtxnp::P3 e1, rtxnp::P3 e2) {
    float u = -1.0f, v = -1.0f, u2 = -2.0f, v2 = -2.0f;
    const int region = rtxnp::triangle_weights(ap, e1, e2, u, v);
    const float d2 = rtxnp::triangle_d2(ap, e1, e2, u2, v2);
    (void)d2;
    CHECK(region == rtxsd::triangle_region(ap, e1, e2), "triangle_region differs from triangle_weights");
    CHECK(region == restated_region(ap, e1, e2), "region %d, the restated chain says %d", region, restated_region(ap, e1, e2));
    CHECK(memcmp(&u, &u2, 4) == 0 && memcmp(&v, &v2, 4) == 0, "region %d: (u, v) differ from triangle_d2's", region);
    if (region >= 0 && region < 7) region_seen[region]++;
    switch (region) {
        case 0: CHECK(u == 0.0f && v == 0.0f, "vertex a: (%g, %g)", u, v); break;
        case 1: CHECK(u == 1.0f && v == 0.0f, "vertex b: (%g, %g)", u, v); break;
        case 2: CHECK(u == 0.0f && v == 1.0f, "vertex c: (%g, %g)", u, v); break;
        case 3: CHECK(v == 0.0f, "edge ab: v = %g", v); break;
        case 5: CHECK(u == 0.0f, "edge ac: u = %g", u); break;
        case 4: CHECK(u == 1.0f - v, "edge bc: u = %g, v = %g", u, v); break;
        case 6: break;
        default: CHECK(false, "region %d", region);
    }
    CHECK(rtxsd::region_feature(region) == (region == 6 ? 1 : region >= 3 ? 2 : 3), "feature of region %d", region);
    region_points++;
}
// points of every Voronoi region of triangle (0, e1, e2) and exactly on every border between two of them: the lines through an edge's end
// perpendicular to it (vertex | edge), the edges' lines above the plane (edge | face), the corners' bisecting rays
static void region_triangle(rtxnp::P3 e1, rtxnp::P3 e2) {
    using namespace rtxnp;
    const P3 a = mk(0.0f, 0.0f, 0.0f), b = e1, c = e2;
    const P3 nrm = mk(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
    const P3 vert[3] = { a, b, c };
    const float lift[5] = { 0.0f, 0.25f, -0.25f, 3.0f, -1e-3f }, along[9] = { -2.0f, -1.0f, -0.5f, 0.0f, 0.25f, 0.5f, 1.0f, 1.5f, 3.0f };
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {
        if (i == j) continue;
        const P3 p = vert[i], q = vert[j], d = sub(q, p);
        // in-plane direction perpendicular to the edge p -> q
        const P3 perp = mk(d.y * nrm.z - d.z * nrm.y, d.z * nrm.x - d.x * nrm.z, d.x * nrm.y - d.y * nrm.x);
        for (float s : along) for (float t : along) for (float h : lift) {
            // on the line through p + s d, moved t across the edge and h off the plane: s in {0, 1} is a vertex | edge border, t = 0 an edge | face one
            const P3 x = add(add(add(p, scale(d, s)), scale(perp, t)), scale(nrm, h));
            region_point(x, e1, e2);
        }
    }
    for (int k = 0; k < 400; k++) region_point(mk(3.0f * rndf(), 3.0f * rndf(), 3.0f * rndf()), e1, e2);
}

int main(int argc, char ** argv) {
    const std::string meshes = argc > 1 ? argv[1] : "../../tests/golden/meshes";
    std::vector<Mesh> shapes;
    { Mesh m; m.name = "one triangle"; m.pos = { 0, 0, 0, 1, 0, 0, 0, 1, 0 }; m.idx = { 0, 1, 2 }; identity_slots(m); shapes.push_back(m); }
    shapes.push_back(soup("85 triangles", 85, 40));
    shapes.push_back(soup("86 triangles", 86, 40));
    shapes.push_back(grid("255 vertices", 15, 17));
    shapes.push_back(grid("256 vertices", 16, 16));
    shapes.push_back(grid("257 vertices", 257, 1));
    shapes.push_back(fan("fan 65", 65));
    shapes.push_back(fan("fan 257", 257));
    for (const char * name : { "icosphere", "Torus", "Monkey", "Rock", "Cube", "Diamond" }) {
        Mesh m; m.name = name;
        const bool ok = load_obj(meshes + "/" + name + ".obj", m);
        CHECK(ok, "%s/%s.obj could not be read", meshes.c_str(), name);
        if (ok) shapes.push_back(m);
    }
    for (const Mesh & m : shapes) run(m);

    // one triangle: every edge is a boundary edge and equals the unit face normal bit for bit; the vertex records are angle * normal
    {
        Mesh m; m.name = "boundary"; m.pos = { 0.1f, 0.2f, 0.3f, 1.3f, 0.1f, -0.2f, 0.4f, 1.7f, 0.6f }; m.idx = { 0, 1, 2 }; identity_slots(m);
        const Tables t = run(m);
        float rec[16]; rtxsd::triangle_record(m.idx.data(), m.pos.data(), 0, 3, rec);
        for (int k = 0; k < 3; k++) CHECK(same_bits(&t.edge[4 * k], rec, 3), "boundary edge %d is not the unit face normal", k);
        for (int k = 0; k < 3; k++) CHECK(same_bits(&t.vert[4 * k], &rec[4 + 4 * k], 3), "vertex %d of one triangle is not its corner vector", k);
        const double sum = (double)rec[7] + rec[11] + rec[15];
        CHECK(fabs(sum - 3.14159265358979) < 1e-5, "the corner angles add up to %.9g", sum);
        const double len = sqrt((double)rec[0] * rec[0] + (double)rec[1] * rec[1] + (double)rec[2] * rec[2]);
        CHECK(fabs(len - 1.0) <= ldexp(1.0, -22), "unit normal of length %.9g", len);
    }
    // a non-manifold edge of three faces around the edge (0, 1); two coincident opposite faces; an unused vertex
    {
        Mesh m; m.name = "non-manifold"; m.pos = { 0, 0, 0, 1, 0, 0, 0.5f, 1, 0, 0.5f, -0.3f, 1, 0.5f, -1, -0.4f, 9, 9, 9 };
        m.idx = { 0, 1, 2, 0, 1, 3, 1, 0, 4 }; identity_slots(m);
        const Tables t = run(m);
        float want[3] = { 0.0f, 0.0f, 0.0f };
        for (int q = 0; q < 3; q++) { float rec[16]; rtxsd::triangle_record(m.idx.data(), m.pos.data(), (uint32_t)q, m.V(), rec); for (int a = 0; a < 3; a++) want[a] += rec[a]; }
        CHECK(same_bits(&t.edge[0], want, 3), "edge ab of slot 0 is not the sum of the three faces");
        CHECK(same_bits(&t.edge[12], want, 3), "edge ab of slot 1 is not the sum of the three faces");
        CHECK(same_bits(&t.edge[24], want, 3), "edge ab of slot 2 (reversed) is not the sum of the three faces");
        CHECK(all_zero_bits(&t.vert[20], 4), "an unused vertex has a pseudonormal");
    }
    {
        Mesh m; m.name = "coincident opposite"; m.pos = { 0, 0, 0, 1, 0, 0, 0, 1, 0 }; m.idx = { 0, 1, 2, 0, 2, 1 }; identity_slots(m);
        const Tables t = run(m);
        for (size_t k = 0; k < t.edge.size(); k++) CHECK(t.edge[k] == 0.0f, "two coincident opposite faces: edge component %zu = %g", k, t.edge[k]);
        for (size_t k = 0; k < t.vert.size(); k++) CHECK(t.vert[k] == 0.0f, "two coincident opposite faces: vertex component %zu = %g", k, t.vert[k]);
    }
    // pad triangles in the topology, pad slots and repeated slots in the slot table
    const Mesh base = grid("rules", 9, 7);
    {
        Mesh m = base; m.name = "padded";
        std::vector<int32_t> idx;
        const int32_t bad[5] = { -1, m.V(), m.V() + 7, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max() };
        for (int32_t t = 0; t < base.T(); t++) {
            if (t % 5 == 0) { const int32_t b = bad[(t / 5) % 5]; for (int k = 0; k < 3; k++) idx.push_back(k == (t / 5) % 3 ? b : base.idx[3 * t + k]); }
            idx.insert(idx.end(), { base.idx[3 * t], base.idx[3 * t + 1], base.idx[3 * t + 2] });
        }
        idx.insert(idx.end(), { -1, -1, -1 });
        m.idx = idx;
        m.slots = base.idx;
        m.slots.insert(m.slots.end(), { -1, -1, -1, 3, -1, 4, base.idx[0], base.idx[1], base.idx[2], base.idx[0], base.idx[1], base.idx[2], m.V(), 0, 1 });
        const Tables t = run(m), clean = run(base);
        CHECK(same_bits(t.vert.data(), clean.vert.data(), clean.vert.size()), "padding changed the vertex table");
        CHECK(same_bits(t.edge.data(), clean.edge.data(), clean.edge.size()), "padding changed the edge table");
        const size_t S0 = (size_t)base.S();
        CHECK(all_zero_bits(&t.edge[12 * S0], 12), "a pad slot has edge records");
        CHECK(all_zero_bits(&t.edge[12 * (S0 + 1)], 4) && all_zero_bits(&t.edge[12 * (S0 + 1) + 4], 4), "edges with a pad vertex have records");
        CHECK(same_bits(&t.edge[12 * (S0 + 2)], &t.edge[0], 12) && same_bits(&t.edge[12 * (S0 + 3)], &t.edge[0], 12), "repeated slots have other records than their twin");
        CHECK(all_zero_bits(&t.edge[12 * (S0 + 4)], 4) && all_zero_bits(&t.edge[12 * (S0 + 4) + 8], 4), "edges with a vertex beyond the table have records");
    }
    { Mesh m = base; m.name = "vertex twice"; m.idx.insert(m.idx.begin() + 30, { 4, 4, 9 }); m.slots = m.idx; run(m); }
    { Mesh m = base; m.name = "all invalid"; for (size_t k = 0; k < m.idx.size(); k += 3) m.idx[k + (k / 3) % 3] = (k / 3) % 2 ? -1 : m.V();
      const Tables t = run(m); CHECK(all_zero_bits(t.vert.data(), t.vert.size()) && all_zero_bits(t.edge.data(), t.edge.size()), "an all-invalid topology has records"); }
    // hostile floats
    {
        const float hostile[][3] = { { NAN, NAN, NAN }, { INFINITY, 0.0f, 0.0f }, { 0.5f, -INFINITY, 0.25f }, { 3e38f, 3e38f, -3e38f }, { -3e38f, 0.1f, 0.2f },
                                     { 1e-41f, -1e-42f, 1e-45f }, { -0.0f, -0.0f, -0.0f }, { NAN, INFINITY, -3e38f } };
        for (size_t h = 0; h < sizeof(hostile) / sizeof(hostile[0]); h++) {
            Mesh m = base; m.name = "hostile " + std::to_string(h);
            memcpy(&m.pos[3 * (size_t)((11 + 5 * h) % (size_t)m.V())], hostile[h], 12);
            run(m);
        }
        Mesh m = base; m.name = "all hostile";
        for (int32_t v = 0; v < m.V(); v++) memcpy(&m.pos[3 * (size_t)v], hostile[v % 8], 12);
        run(m);
        for (int e : { -60, -20, 20, 40, 62 }) { Mesh s = base; s.name = "scaled"; for (float & x : s.pos) x = ldexpf(x, e); run(s); }
    }
    // the region
    {
        using rtxnp::mk;
        region_triangle(mk(1.0f, 0.0f, 0.0f), mk(0.0f, 1.0f, 0.0f));
        region_triangle(mk(2.0f, 0.0f, 0.0f), mk(0.5f, 1.5f, 0.0f));
        region_triangle(mk(1.0f, 0.25f, -0.5f), mk(-0.75f, 1.0f, 0.5f));
        region_triangle(mk(4.0f, 0.0f, 0.0f), mk(-2.0f, 0.5f, 0.0f));          // obtuse at a
        region_triangle(mk(1.0f, 0.0f, 0.0f), mk(3.0f, 0.125f, 0.0f));         // obtuse at b, thin
        for (int r = 0; r < 7; r++) CHECK(region_seen[r] > 0, "region %d never taken", r);
        // degenerate and hostile triangles: a region and the weights of triangle_d2 all the same
        region_point(mk(0.5f, 0.5f, 0.5f), mk(0.0f, 0.0f, 0.0f), mk(0.0f, 0.0f, 0.0f));
        region_point(mk(0.5f, 0.5f, 0.5f), mk(1.0f, 0.0f, 0.0f), mk(2.0f, 0.0f, 0.0f));
        region_point(mk(NAN, 0.5f, 0.5f), mk(1.0f, 0.0f, 0.0f), mk(0.0f, 1.0f, 0.0f));
        region_point(mk(0.5f, 0.5f, 0.5f), mk(NAN, 0.0f, 0.0f), mk(0.0f, INFINITY, 0.0f));
    }
    // the sign rule's scalars
    CHECK(rtxsd::signed_distance(0.0f, true) == 0.0f && !signbit(rtxsd::signed_distance(0.0f, true)), "d2 == 0 is not +0");
    CHECK(rtxsd::signed_distance(4.0f, true) == -2.0f && rtxsd::signed_distance(4.0f, false) == 2.0f, "signed_distance");
    if (failures) { printf("side_check: %d checks failed\n", failures); return 1; }
    printf("side_check: ok (%d region points)\n", region_points);
    return 0;
}
