// normals_check.cpp — the device plan of rtx_set_blas_topology / rtx_blas_vertex_normals run on the CPU through the functions the kernels call
// (rtx_normals_math.h): keys, a sort, the lower-bound offsets, pass 1 (face vectors), pass 2 (the sum per vertex) — compared bit for bit with
// the plain scatter loop rtxh_vertex_normals is written as, on the shapes tests/test_gpu_vertex_normals.py uses and on hostile floats.
// For every mesh: each corner of a valid triangle lies in exactly one vertex's list, no list entry is the corner of an invalid triangle,
// every offset lies in [0, 3T].  Built with the host sanitizers (make normals_check): no GPU, no ROCm.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <limits>
#include <string>
#include <vector>
#include "rtx_normals_math.h"

struct Face4 { float x, y, z, w; };                     // the float4 of the device
struct Mesh { std::string name; std::vector<float> pos; std::vector<int32_t> idx; int32_t T() const { return (int32_t)(idx.size() / 3); } int32_t V() const { return (int32_t)(pos.size() / 3); } };

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("normals_check: FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf() { return (float)rnd() / 16777216.0f * 2.0f - 1.0f; }

// the host twin's loop: over triangles, over corners, acc[v] += f, then normalise
static std::vector<float> scatter_loop(const Mesh & m) {
    const int32_t T = m.T(), V = m.V();
    std::vector<float> acc((size_t)3 * V, 0.0f), out((size_t)3 * V);
    for (int32_t t = 0; t < T; t++) {
        const int32_t * const tri = &m.idx[3 * (size_t)t];
        if (!rtxn::valid_triangle(tri[0], tri[1], tri[2], V)) continue;
        float f[3];
        rtxn::face_vector(&m.pos[3 * (size_t)tri[0]], &m.pos[3 * (size_t)tri[1]], &m.pos[3 * (size_t)tri[2]], f);
        for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) acc[3 * (size_t)tri[k] + a] += f[a];
    }
    for (int32_t v = 0; v < V; v++) rtxn::normalise(&acc[3 * (size_t)v], &out[3 * (size_t)v]);
    return out;
}

// the device plan, launch by launch; the sort gets its input reversed (the key is a total order: any correct sort gives one result)
static std::vector<float> device_plan(const Mesh & m) {
    const int32_t T = m.T(), V = m.V();
    const uint32_t n = 3u * (uint32_t)T;
    // k_normals_keys
    std::vector<int32_t> indices(n); std::vector<uint64_t> keys(n);
    for (uint32_t c = 0; c < n; c++) {
        const uint32_t t = c / 3u;
        const int32_t tri[3] = { m.idx[3 * (size_t)t], m.idx[3 * (size_t)t + 1], m.idx[3 * (size_t)t + 2] };
        indices[c] = tri[c - 3u * t];
        keys[c] = rtxn::corner_key(tri, c, V);
    }
    const unsigned int bits = rtxn::key_bits(V);
    CHECK(bits >= 33 && bits <= 64, "%s: key bits %u", m.name.c_str(), bits);
    for (uint32_t c = 0; c < n; c++) CHECK(bits == 64 || (keys[c] >> bits) == 0, "%s: key of corner %u has bits above %u", m.name.c_str(), c, bits);
    // the radix sort
    std::reverse(keys.begin(), keys.end());
    std::sort(keys.begin(), keys.end());
    // k_normals_offsets
    std::vector<uint32_t> offset((size_t)V + 1);
    for (uint32_t v = 0; v <= (uint32_t)V; v++) offset[v] = rtxn::lower_bound(keys.data(), n, (uint64_t)v << 32);
    // what the lists hold
    std::vector<int> seen(n, 0);
    for (uint32_t v = 0; v <= (uint32_t)V; v++) CHECK(offset[v] <= n, "%s: offset[%u] = %u beyond %u", m.name.c_str(), v, offset[v], n);
    CHECK(offset[0] == 0, "%s: offset[0] = %u", m.name.c_str(), offset[0]);
    for (int32_t v = 0; v < V; v++) {
        CHECK(offset[v] <= offset[v + 1], "%s: offsets of vertex %d descend", m.name.c_str(), v);
        for (uint32_t k = offset[v]; k < offset[v + 1] && k < n; k++) {
            const uint32_t c = (uint32_t)keys[k];
            CHECK(c < n, "%s: corner %u beyond %u", m.name.c_str(), c, n);
            if (c >= n) continue;
            const int32_t * const tri = &m.idx[3 * (size_t)(c / 3u)];
            CHECK(rtxn::valid_triangle(tri[0], tri[1], tri[2], V), "%s: list of vertex %d holds corner %u of an invalid triangle", m.name.c_str(), v, c);
            CHECK(tri[c % 3u] == v, "%s: list of vertex %d holds corner %u of vertex %d", m.name.c_str(), v, c, tri[c % 3u]);
            CHECK(k == offset[v] || (uint32_t)keys[k - 1] < c, "%s: list of vertex %d is not ascending", m.name.c_str(), v);
            seen[c]++;
        }
    }
    for (uint32_t c = 0; c < n; c++) {
        const int32_t * const tri = &m.idx[3 * (size_t)(c / 3u)];
        const int want = rtxn::valid_triangle(tri[0], tri[1], tri[2], V) ? 1 : 0;
        CHECK(seen[c] == want, "%s: corner %u lies in %d lists, expected %d", m.name.c_str(), c, seen[c], want);
    }
    // k_normals_faces
    std::vector<Face4> face((size_t)T);
    for (int32_t t = 0; t < T; t++) {
        float f[3];
        rtxn::triangle_face(indices.data(), m.pos.data(), (uint32_t)t, V, f);
        face[t] = Face4{ f[0], f[1], f[2], 0.0f };
    }
    // k_normals_sum
    std::vector<float> out((size_t)3 * V);
    for (int32_t v = 0; v < V; v++) rtxn::vertex_normal(keys.data(), offset[v], offset[v + 1], face.data(), &out[3 * (size_t)v]);
    return out;
}

// per vertex: did the scatter loop meet a subnormal product, face component or partial sum on the way to its sum?
static bool subnormal(float x) { return x != 0.0f && fabsf(x) < std::numeric_limits<float>::min(); }
static std::vector<char> subnormal_seen(const Mesh & m) {
    const int32_t T = m.T(), V = m.V();
    std::vector<char> seen((size_t)V, 0); std::vector<float> acc((size_t)3 * V, 0.0f);
    for (int32_t t = 0; t < T; t++) {
        const int32_t * const tri = &m.idx[3 * (size_t)t];
        if (!rtxn::valid_triangle(tri[0], tri[1], tri[2], V)) continue;
        const float * const p0 = &m.pos[3 * (size_t)tri[0]], * const p1 = &m.pos[3 * (size_t)tri[1]], * const p2 = &m.pos[3 * (size_t)tri[2]];
        float e1[3], e2[3], f[3]; bool sub = false;
        for (int a = 0; a < 3; a++) { e1[a] = p1[a] - p0[a]; e2[a] = p2[a] - p0[a]; sub = sub || subnormal(e1[a]) || subnormal(e2[a]); }
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) sub = sub || subnormal(e1[a] * e2[b]);
        rtxn::face_vector(p0, p1, p2, f);
        for (int a = 0; a < 3; a++) sub = sub || subnormal(f[a]);
        for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) { float & s = acc[3 * (size_t)tri[k] + a]; s += f[a]; if (sub || subnormal(s)) seen[tri[k]] = 1; }
    }
    return seen;
}

static void run(const Mesh & m, bool expect_all_zero = false) {
    CHECK(m.T() >= 1 && m.V() >= 1, "%s: empty", m.name.c_str());
    const std::vector<float> a = scatter_loop(m), b = device_plan(m);
    CHECK(a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * 4) == 0, "%s: the device plan and the scatter loop differ", m.name.c_str());
    for (size_t k = 0; k < a.size(); k++) CHECK(rtxu::is_finite(a[k]), "%s: component %zu is not finite", m.name.c_str(), k);
    for (int32_t v = 0; v < m.V(); v++) {
        const float * const n = &a[3 * (size_t)v];
        uint32_t u[3]; memcpy(u, n, 12);
        const bool zero = u[0] == 0 && u[1] == 0 && u[2] == 0;
        const double len = sqrt((double)n[0] * n[0] + (double)n[1] * n[1] + (double)n[2] * n[2]);
        CHECK(zero || fabs(1.0 - len) <= ldexp(1.0, -22), "%s: normal %d has length %.9g", m.name.c_str(), v, len);
        if (expect_all_zero) CHECK(zero, "%s: normal %d is not +0 +0 +0", m.name.c_str(), v);
    }
}

// ---- the shapes ----------------------------------------------------------------------------------------------------------------------------
// V random vertices, T random triangles over them
static Mesh soup(const char * name, int32_t T, int32_t V) {
    Mesh m; m.name = name;
    for (int32_t k = 0; k < 3 * V; k++) m.pos.push_back(rndf());
    for (int32_t k = 0; k < 3 * T; k++) m.idx.push_back((int32_t)(rnd() % (uint32_t)V));
    return m;
}
// a fan: vertex 0 in the middle of `valence` triangles over a ring
static Mesh fan(const char * name, int32_t valence) {
    Mesh m; m.name = name;
    m.pos = { 0.0f, 0.3f, 0.0f };
    for (int32_t k = 0; k < valence; k++) { const float a = 6.2831853f * (float)k / (float)valence; m.pos.push_back(cosf(a)); m.pos.push_back(0.05f * rndf()); m.pos.push_back(sinf(a)); }
    for (int32_t k = 0; k < valence; k++) { m.idx.push_back(0); m.idx.push_back(1 + (k + 1) % valence); m.idx.push_back(1 + k); }
    return m;
}
// a closed grid (torus) of `rows` x `cols` vertices, two triangles per cell: valence 6 everywhere
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
    return m;
}
// an OBJ file's v lines and f lines (polygons as fans from their first vertex), the way the tests index the golden meshes
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
    return !m.pos.empty() && !m.idx.empty();
}

int main(int argc, char ** argv) {
    const std::string meshes = argc > 1 ? argv[1] : "../../tests/golden/meshes";
    // the lower bound on its own: every key and every gap of a small sorted list
    {
        std::vector<uint64_t> keys;
        for (uint32_t n = 0; n <= 70; n++) {
            for (uint64_t q = 0; q <= 2 * (uint64_t)n + 2; q++) {
                const uint32_t got = rtxn::lower_bound(keys.data(), n, q);
                const uint32_t want = (uint32_t)(std::lower_bound(keys.begin(), keys.end(), q) - keys.begin());
                CHECK(got == want, "lower_bound(n = %u, key = %llu) = %u, expected %u", n, (unsigned long long)q, got, want);
            }
            keys.push_back(2 * (uint64_t)n + 1);
        }
        CHECK(rtxn::key_bits(1) == 33 && rtxn::key_bits(255) == 40 && rtxn::key_bits(256) == 41 && rtxn::key_bits(0x7fffffff) == 63, "key_bits");
    }
    std::vector<Mesh> shapes;
    { Mesh m; m.name = "one triangle"; m.pos = { 0, 0, 0, 1, 0, 0, 0, 1, 0 }; m.idx = { 0, 1, 2 }; shapes.push_back(m); }
    shapes.push_back(soup("85 triangles", 85, 40));
    shapes.push_back(soup("86 triangles", 86, 40));
    shapes.push_back(grid("255 vertices", 15, 17));
    shapes.push_back(grid("256 vertices", 16, 16));
    shapes.push_back(grid("257 vertices", 257, 1));
    shapes.push_back(fan("fan 65", 65));
    shapes.push_back(fan("fan 257", 257));
    for (const char * name : { "icosphere", "Torus", "Monkey", "Rock", "Cube" }) {
        Mesh m; m.name = name;
        const bool ok = load_obj(meshes + "/" + name + ".obj", m);
        CHECK(ok, "%s/%s.obj could not be read", meshes.c_str(), name);
        if (ok) shapes.push_back(m);
    }
    for (const Mesh & m : shapes) run(m);
    { Mesh m; m.name = "one vertex"; m.pos = { 1, 2, 3 }; m.idx = { 0, 0, 0 }; run(m, true); }

    // the rules: padding and bad indices, a triangle that names a vertex twice, an unused vertex, nothing valid
    const Mesh base = grid("rules", 9, 7);
    {
        Mesh m = base; m.name = "padded";
        const int32_t bad[5] = { -1, m.V(), m.V() + 7, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max() };
        std::vector<int32_t> idx;
        for (int32_t t = 0; t < base.T(); t++) {
            if (t % 5 == 0) { const int32_t b = bad[(t / 5) % 5]; const int32_t tri[3] = { base.idx[3 * t], base.idx[3 * t + 1], base.idx[3 * t + 2] };
                              for (int k = 0; k < 3; k++) idx.push_back(k == (t / 5) % 3 ? b : tri[k]); }
            idx.insert(idx.end(), { base.idx[3 * t], base.idx[3 * t + 1], base.idx[3 * t + 2] });
        }
        idx.insert(idx.end(), { -1, -1, -1, -1, -1, -1 });
        m.idx = idx;
        run(m);
        const std::vector<float> a = scatter_loop(m), b = scatter_loop(base);
        CHECK(memcmp(a.data(), b.data(), a.size() * 4) == 0, "padding changed the normals");
    }
    { Mesh m = base; m.name = "vertex twice"; m.idx.insert(m.idx.begin() + 30, { 4, 4, 9 }); run(m);
      const std::vector<float> a = scatter_loop(m), b = scatter_loop(base); CHECK(memcmp(a.data(), b.data(), a.size() * 4) == 0, "a zero-area triangle changed the normals"); }
    { Mesh m = base; m.name = "unused vertex"; m.pos.insert(m.pos.end(), { 5.0f, 5.0f, 5.0f }); run(m);
      const std::vector<float> a = scatter_loop(m); uint32_t u[3]; memcpy(u, &a[a.size() - 3], 12); CHECK(u[0] == 0 && u[1] == 0 && u[2] == 0, "an unused vertex has a normal"); }
    { Mesh m = base; m.name = "all invalid"; for (size_t k = 0; k < m.idx.size(); k += 3) m.idx[k + (k / 3) % 3] = (k / 3) % 2 ? -1 : m.V(); run(m, true); }

    // hostile floats planted at single vertices: the others keep their bytes
    {
        const float hostile[][3] = { { NAN, NAN, NAN }, { INFINITY, 0.0f, 0.0f }, { 0.5f, -INFINITY, 0.25f }, { 3e38f, 3e38f, -3e38f }, { -3e38f, 0.1f, 0.2f },
                                     { 1e-41f, -1e-42f, 1e-45f }, { -0.0f, -0.0f, -0.0f }, { NAN, INFINITY, -3e38f } };
        const std::vector<float> clean = scatter_loop(base);
        for (size_t h = 0; h < sizeof(hostile) / sizeof(hostile[0]); h++) {
            Mesh m = base; m.name = "hostile " + std::to_string(h);
            const int32_t bad = (int32_t)(11 + 5 * h) % m.V();
            memcpy(&m.pos[3 * (size_t)bad], hostile[h], 12);
            run(m);
            std::vector<char> touched((size_t)m.V(), 0);
            for (int32_t t = 0; t < m.T(); t++) if (m.idx[3 * t] == bad || m.idx[3 * t + 1] == bad || m.idx[3 * t + 2] == bad) for (int k = 0; k < 3; k++) touched[m.idx[3 * t + k]] = 1;
            const std::vector<float> a = scatter_loop(m);
            for (int32_t v = 0; v < m.V(); v++) if (!touched[v]) CHECK(memcmp(&a[3 * (size_t)v], &clean[3 * (size_t)v], 12) == 0, "%s: vertex %d is no neighbour and changed", m.name.c_str(), v);
        }
        Mesh m = base; m.name = "all hostile";
        for (int32_t v = 0; v < m.V(); v++) memcpy(&m.pos[3 * (size_t)v], hostile[v % 8], 12);
        run(m);
    }
    // scale: exact powers of two give the same bytes wherever no intermediate value (product, face component, partial sum) is subnormal
    {
        const std::vector<float> one = scatter_loop(base);
        for (int e : { -60, 40 }) {
            Mesh m = base; m.name = "scaled";
            for (float & x : m.pos) x = ldexpf(x, e);
            run(m);
            const std::vector<char> sub = subnormal_seen(m);
            const std::vector<float> a = scatter_loop(m);
            int compared = 0;
            for (int32_t v = 0; v < m.V(); v++) {
                uint32_t u[3]; memcpy(u, &a[3 * (size_t)v], 12);
                CHECK(u[0] || u[1] || u[2], "scaling by 2^%d: vertex %d has a zero normal", e, v);
                if (sub[v]) continue;
                compared++;
                CHECK(memcmp(&a[3 * (size_t)v], &one[3 * (size_t)v], 12) == 0, "scaling by 2^%d changed the normal of vertex %d", e, v);
            }
            // at 2^-60 a product below 2^-6 of the unscaled mesh is already subnormal: few vertices qualify; at 2^40 all do
            CHECK(e < 0 ? compared > 0 : compared == m.V(), "scaling by 2^%d: only %d of %d vertices compared", e, compared, m.V());
        }
    }
    if (failures) { printf("normals_check: %d checks failed\n", failures); return 1; }
    printf("normals_check: ok\n");
    return 0;
}
