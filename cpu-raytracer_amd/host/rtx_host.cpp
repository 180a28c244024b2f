// rtx_host.cpp — librtx_host.so: host-side callers of the render path (see include/rtx_host.h).
//
// Compiled with -ffp-contract=off: the functions that mirror Scene::update must reproduce the
// reference's scalar Vector3 / Matrix4 / Quaternion arithmetic bit for bit (tests compare against
// matrices and TLAS nodes dumped from the real reference), and those classes evaluate
// left-to-right with plain mul/add (Vector3.h:33-43, Matrix4.h:31-68, Quaternion.h:128-133).
#include "../../include/rtx_host.h"
#include "../csrc/rtx_update_math.h"
#include "../csrc/rtx_refit_math.h"
#include "../csrc/rtx_build_math.h"
#include "../csrc/rtx_normals_math.h"
#include "../csrc/rtx_texmip_math.h"
#include "../csrc/rtx_query_sort_math.h"
#include "../csrc/rtx_nearest_math.h"
#include "../csrc/rtx_side_math.h"
#include "../csrc/rtx_hits_math.h"
#include "../csrc/rtx_overlap_math.h"
#include "../csrc/rtx_capsule_math.h"
#include "../csrc/rtx_sweep_math.h"
#include "../csrc/rtx_boxsweep_math.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

namespace {

struct V { float x, y, z; };
inline V mk(float x, float y, float z) { V r = { x, y, z }; return r; }
inline V operator+(V a, V b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
inline V operator-(V a, V b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
inline V operator*(V a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
inline V operator*(float s, V a) { return mk(a.x * s, a.y * s, a.z * s); }
inline float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }                                 // Vector3.h:33-35
inline V cross(V a, V b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }   // Vector3.h:37-43
inline V vmin(V a, V b) { return mk(a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y, a.z < b.z ? a.z : b.z); }
inline V vmax(V a, V b) { return mk(a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y, a.z > b.z ? a.z : b.z); }
inline float comp(V a, int d) { return d == 0 ? a.x : d == 1 ? a.y : a.z; }

// Quaternion * Vector3, Quaternion.h:128-133
inline V rotate(const float q4[4], V v) {
    V q = mk(q4[0], q4[1], q4[2]);
    float w = q4[3];
    return 2.0f * dot(q, v) * q + (w * w - dot(q, q)) * v + 2.0f * w * cross(q, v);
}

// Matrix4(i, j) = cells[i + 4j], Matrix4.h:19-23
inline V m_position(const float * c, V p) {    // scalar Matrix4::transform_position, Matrix4.h:31-37
    return mk(c[0] * p.x + c[1] * p.y + c[2]  * p.z + c[3],
              c[4] * p.x + c[5] * p.y + c[6]  * p.z + c[7],
              c[8] * p.x + c[9] * p.y + c[10] * p.z + c[11]);
}
inline V m_direction(const float * c, V d) {   // scalar Matrix4::transform_direction, Matrix4.h:62-68
    return mk(c[0] * d.x + c[1] * d.y + c[2]  * d.z,
              c[4] * d.x + c[5] * d.y + c[6]  * d.z,
              c[8] * d.x + c[9] * d.y + c[10] * d.z);
}

// Transform::calc_world_matrix, Transform.h:13-43 (cells not written keep the identity of Matrix4())
void world_matrix(const float p[3], const float r[4], float * c) {
    memset(c, 0, 64); c[0] = c[5] = c[10] = c[15] = 1.0f;
    float xx = r[0] * r[0], yy = r[1] * r[1], zz = r[2] * r[2];
    float xz = r[0] * r[2], xy = r[0] * r[1], yz = r[1] * r[2];
    float wx = r[3] * r[0], wy = r[3] * r[1], wz = r[3] * r[2];
    c[0 + 4 * 0] = 1.0f - 2.0f * (yy + zz); c[0 + 4 * 1] = 2.0f * (xy + wz);        c[0 + 4 * 2] = 2.0f * (xz - wy);
    c[1 + 4 * 0] = 2.0f * (xy - wz);        c[1 + 4 * 1] = 1.0f - 2.0f * (xx + zz); c[1 + 4 * 2] = 2.0f * (yz + wx);
    c[2 + 4 * 0] = 2.0f * (xz + wy);        c[2 + 4 * 1] = 2.0f * (yz - wx);        c[2 + 4 * 2] = 1.0f - 2.0f * (xx + yy);
    c[3 + 4 * 0] = p[0]; c[3 + 4 * 1] = p[1]; c[3 + 4 * 2] = p[2];
}

// Matrix4::invert, Matrix4.h:88-138: adjugate by cofactors.  Row k of the table lists the six signed
// triple products of inv[k] in the order the reference sums them (left to right).
const signed char INV_TERMS[16][6][4] = {
    { { 1, 5, 10, 15 }, { -1, 5, 11, 14 }, { -1, 9, 6, 15 }, { 1, 9, 7, 14 }, { 1, 13, 6, 11 }, { -1, 13, 7, 10 } },
    { { -1, 1, 10, 15 }, { 1, 1, 11, 14 }, { 1, 9, 2, 15 }, { -1, 9, 3, 14 }, { -1, 13, 2, 11 }, { 1, 13, 3, 10 } },
    { { 1, 1, 6, 15 }, { -1, 1, 7, 14 }, { -1, 5, 2, 15 }, { 1, 5, 3, 14 }, { 1, 13, 2, 7 }, { -1, 13, 3, 6 } },
    { { -1, 1, 6, 11 }, { 1, 1, 7, 10 }, { 1, 5, 2, 11 }, { -1, 5, 3, 10 }, { -1, 9, 2, 7 }, { 1, 9, 3, 6 } },
    { { -1, 4, 10, 15 }, { 1, 4, 11, 14 }, { 1, 8, 6, 15 }, { -1, 8, 7, 14 }, { -1, 12, 6, 11 }, { 1, 12, 7, 10 } },
    { { 1, 0, 10, 15 }, { -1, 0, 11, 14 }, { -1, 8, 2, 15 }, { 1, 8, 3, 14 }, { 1, 12, 2, 11 }, { -1, 12, 3, 10 } },
    { { -1, 0, 6, 15 }, { 1, 0, 7, 14 }, { 1, 4, 2, 15 }, { -1, 4, 3, 14 }, { -1, 12, 2, 7 }, { 1, 12, 3, 6 } },
    { { 1, 0, 6, 11 }, { -1, 0, 7, 10 }, { -1, 4, 2, 11 }, { 1, 4, 3, 10 }, { 1, 8, 2, 7 }, { -1, 8, 3, 6 } },
    { { 1, 4, 9, 15 }, { -1, 4, 11, 13 }, { -1, 8, 5, 15 }, { 1, 8, 7, 13 }, { 1, 12, 5, 11 }, { -1, 12, 7, 9 } },
    { { -1, 0, 9, 15 }, { 1, 0, 11, 13 }, { 1, 8, 1, 15 }, { -1, 8, 3, 13 }, { -1, 12, 1, 11 }, { 1, 12, 3, 9 } },
    { { 1, 0, 5, 15 }, { -1, 0, 7, 13 }, { -1, 4, 1, 15 }, { 1, 4, 3, 13 }, { 1, 12, 1, 7 }, { -1, 12, 3, 5 } },
    { { -1, 0, 5, 11 }, { 1, 0, 7, 9 }, { 1, 4, 1, 11 }, { -1, 4, 3, 9 }, { -1, 8, 1, 7 }, { 1, 8, 3, 5 } },
    { { -1, 4, 9, 14 }, { 1, 4, 10, 13 }, { 1, 8, 5, 14 }, { -1, 8, 6, 13 }, { -1, 12, 5, 10 }, { 1, 12, 6, 9 } },
    { { 1, 0, 9, 14 }, { -1, 0, 10, 13 }, { -1, 8, 1, 14 }, { 1, 8, 2, 13 }, { 1, 12, 1, 10 }, { -1, 12, 2, 9 } },
    { { -1, 0, 5, 14 }, { 1, 0, 6, 13 }, { 1, 4, 1, 14 }, { -1, 4, 2, 13 }, { -1, 12, 1, 6 }, { 1, 12, 2, 5 } },
    { { 1, 0, 5, 10 }, { -1, 0, 6, 9 }, { -1, 4, 1, 10 }, { 1, 4, 2, 9 }, { 1, 8, 1, 6 }, { -1, 8, 2, 5 } },
};

void invert(const float * m, float * out) {
    float inv[16];
    for (int k = 0; k < 16; k++) {
        float acc = 0.0f;
        for (int t = 0; t < 6; t++) {
            const signed char * e = INV_TERMS[k][t];
            float a = m[e[1]]; if (e[0] < 0) a = -a;
            float term = a * m[e[2]] * m[e[3]];
            acc = (t == 0) ? term : acc + term;
        }
        inv[k] = acc;
    }
    memset(out, 0, 64); out[0] = out[5] = out[10] = out[15] = 1.0f;
    float det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    if (det != 0.0f) {
        const float inv_det = 1.0f / det;
        for (int i = 0; i < 16; i++) out[i] = inv[i] * inv_det;
    }
}

struct Box { V mn, mx; };
inline Box empty_box() { Box b; b.mn = mk(INFINITY, INFINITY, INFINITY); b.mx = mk(-INFINITY, -INFINITY, -INFINITY); return b; }
inline void expand(Box & b, const Box & o) { b.mn = vmin(b.mn, o.mn); b.mx = vmax(b.mx, o.mx); }
inline void expand(Box & b, V p) { b.mn = vmin(b.mn, p); b.mx = vmax(b.mx, p); }
inline void fix_if_needed(Box & b) {     // AABB::fix_if_needed, AABB.h:26-32: slabs need a non-zero extent
    if (b.mx.x - b.mn.x < 0.001f) b.mx.x += 0.005f;
    if (b.mx.y - b.mn.y < 0.001f) b.mx.y += 0.005f;
    if (b.mx.z - b.mn.z < 0.001f) b.mx.z += 0.005f;
}
inline float surface_area(const Box & b) {   // AABB.h:34-40
    V d = b.mx - b.mn;
    return 2.0f * (d.x * d.y + d.y * d.z + d.z * d.x);
}

}  // namespace

// =================================================================================================
extern "C" int rtxh_camera_basis(int32_t width, int32_t height, float fov, const float position[3], const float rotation[4], rtx_camera * out) {
    if (!position || !rotation || !out || width <= 0 || height <= 0) return RTX_ERR_INVALID_ARG;
    float half_width = 0.5f * width, half_height = 0.5f * height;          // Camera::resize, Camera.cpp:5-16
    float d = half_width / tanf(0.5f * fov);
    V tl = rotate(rotation, mk(-half_width, half_height, d));              // Camera::update, Camera.cpp:44-47
    V xa = rotate(rotation, mk(1.0f, 0.0f, 0.0f));
    V ya = rotate(rotation, mk(0.0f, -1.0f, 0.0f));
    memcpy(out->position, position, 12);
    out->rotated_top_left_corner[0] = tl.x; out->rotated_top_left_corner[1] = tl.y; out->rotated_top_left_corner[2] = tl.z;
    out->rotated_x_axis[0] = xa.x; out->rotated_x_axis[1] = xa.y; out->rotated_x_axis[2] = xa.z;
    out->rotated_y_axis[0] = ya.x; out->rotated_y_axis[1] = ya.y; out->rotated_y_axis[2] = ya.z;
    return RTX_OK;
}

extern "C" int rtxh_instance_update(const float position[3], const float rotation[4], const float mn[3], const float mx[3],
                                    rtx_instance * out, float out_min[3], float out_max[3]) {
    if (!position || !rotation || !mn || !mx || !out) return RTX_ERR_INVALID_ARG;
    world_matrix(position, rotation, out->world);                            // Mesh::update, Mesh.cpp:9-15
    // AABB::transform, AABB.cpp:55-73
    V bmn = mk(mn[0], mn[1], mn[2]), bmx = mk(mx[0], mx[1], mx[2]);
    V center = 0.5f * (bmn + bmx), extent = 0.5f * (bmx - bmn);
    float absm[16];
    for (int i = 0; i < 16; i++) absm[i] = fabsf(out->world[i]);
    V nc = m_position(out->world, center), ne = m_direction(absm, extent);
    V omn = nc - ne, omx = nc + ne;
    if (out_min) { out_min[0] = omn.x; out_min[1] = omn.y; out_min[2] = omn.z; }
    if (out_max) { out_max[0] = omx.x; out_max[1] = omx.y; out_max[2] = omx.z; }
    invert(out->world, out->world_inv);
    return RTX_OK;
}

extern "C" int rtxh_quaternion_axis_angle(const float axis[3], float angle, float out[4]) {    // Quaternion::axis_angle, Quaternion.h:26-36
    if (!axis || !out) return RTX_ERR_INVALID_ARG;
    float half_angle = 0.5f * angle;
    float sine = sinf(half_angle);
    out[0] = axis[0] * sine; out[1] = axis[1] * sine; out[2] = axis[2] * sine; out[3] = cosf(half_angle);
    return RTX_OK;
}

// ---- Scene::update, Scene.cpp:139-171 ---------------------------------------------------------------------------------
namespace {
struct Q { float x, y, z, w; };
inline Q q_axis_angle(float ax, float ay, float az, float angle) {                 // Quaternion.h:26-36
    float half_angle = 0.5f * angle, sine = sinf(half_angle);
    return Q{ ax * sine, ay * sine, az * sine, cosf(half_angle) };
}
inline Q q_mul(Q l, Q r) {                                                          // operator*(Quaternion, Quaternion&), Quaternion.h:118-125
    return Q{ l.x * r.w + l.w * r.x + l.y * r.z - l.z * r.y,
              l.y * r.w + l.w * r.y + l.z * r.x - l.x * r.z,
              l.z * r.w + l.w * r.z + l.x * r.y - l.y * r.x,
              l.w * r.w - l.x * r.x - l.y * r.y - l.z * r.z };
}
inline Q q_nlerp(Q a, Q b, float t) {                                               // Quaternion::nlerp + normalize
    float one_minus_t = 1.0f - t;
    Q q{ one_minus_t * a.x + t * b.x, one_minus_t * a.y + t * b.y, one_minus_t * a.z + t * b.z, one_minus_t * a.w + t * b.w };
    float inv_length = 1.0f / sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return Q{ q.x * inv_length, q.y * inv_length, q.z * inv_length, q.w * inv_length };
}
}  // namespace

// Camera::update's input half (Camera.cpp:18-39): WASD / shift / space move at 10 units/s, the arrow keys turn at 3 rad/s; each key
// acts on the state the previous key left (position first, then rotation; `right` and `forward` are taken once, before any of it).
extern "C" int rtxh_camera_update(float delta, uint32_t keys, float position[3], float rotation[4]) {
    if (!position || !rotation) return RTX_ERR_INVALID_ARG;
    const float MOVEMENT_SPEED = 10.0f, ROTATION_SPEED = 3.0f;
    const V right = rotate(rotation, mk(1.0f, 0.0f, 0.0f)), forward = rotate(rotation, mk(0.0f, 0.0f, 1.0f));
    V p = mk(position[0], position[1], position[2]);
    if (keys & RTXH_KEY_W) p = p + forward * MOVEMENT_SPEED * delta;
    if (keys & RTXH_KEY_A) p = p - right   * MOVEMENT_SPEED * delta;
    if (keys & RTXH_KEY_S) p = p - forward * MOVEMENT_SPEED * delta;
    if (keys & RTXH_KEY_D) p = p + right   * MOVEMENT_SPEED * delta;
    if (keys & RTXH_KEY_LSHIFT) p.y -= MOVEMENT_SPEED * delta;
    if (keys & RTXH_KEY_SPACE)  p.y += MOVEMENT_SPEED * delta;
    Q r{ rotation[0], rotation[1], rotation[2], rotation[3] };
    if (keys & RTXH_KEY_UP)    r = q_mul(q_axis_angle(right.x, right.y, right.z, -ROTATION_SPEED * delta), r);
    if (keys & RTXH_KEY_DOWN)  r = q_mul(q_axis_angle(right.x, right.y, right.z, +ROTATION_SPEED * delta), r);
    if (keys & RTXH_KEY_LEFT)  r = q_mul(q_axis_angle(0.0f, 1.0f, 0.0f, -ROTATION_SPEED * delta), r);
    if (keys & RTXH_KEY_RIGHT) r = q_mul(q_axis_angle(0.0f, 1.0f, 0.0f, +ROTATION_SPEED * delta), r);
    position[0] = p.x; position[1] = p.y; position[2] = p.z;
    rotation[0] = r.x; rotation[1] = r.y; rotation[2] = r.z; rotation[3] = r.w;
    return RTX_OK;
}

// The animation SCENE_DYNAMIC hard-codes into Scene::update (Scene.cpp:141-155): instances 0..5 move, *time accumulates delta.
extern "C" int rtxh_scene_dynamic_animate(float delta, float * time, float * positions, float * rotations, int32_t instance_count) {
    if (!time || !positions || !rotations || instance_count < 6) return RTX_ERR_INVALID_ARG;
    auto rot = [&](int i) -> Q & { return *reinterpret_cast<Q *>(rotations + 4 * i); };
    float * p = positions;
    rot(0) = q_mul(q_axis_angle(0.0f, 1.0f, 0.0f, delta), rot(0));
    *time += delta;
    const float t = *time;
    p[3 * 1 + 1] = 1.0f + 2.0f * sinf(t);
    p[3 * 2 + 0] -= delta * 0.5f;
    p[3 * 3 + 0] = 6.0f; p[3 * 3 + 1] = 4.0f + 2.0f * sinf(t * 0.5f); p[3 * 3 + 2] = 4.0f + 2.0f * cosf(t * 0.5f);
    rot(3) = q_mul(q_axis_angle(0.0f, 1.0f, 0.0f, delta * 0.5f), rot(3));
    rot(4) = q_mul(q_axis_angle(1.0f, 0.0f, 0.0f, delta), rot(4));
    rot(5) = q_nlerp(Q{ 0.0f, 0.0f, 0.0f, 1.0f }, q_axis_angle(1.0f, 0.0f, 0.0f, (-90.0f) * 3.14159265359f * 0.00555555555f), 0.5f + 0.5f * sinf(t));
    return RTX_OK;
}

// Mesh::update for every instance + TopLevelBVH::build_bvh in one call (the tail of Scene::update, Scene.cpp:166-170).
extern "C" int rtxh_scene_update(rtxh_tlas * tlas, int32_t instance_count, const float * positions, const float * rotations, const int32_t * blas_ids,
                                 const float * blas_root_aabbs, rtx_instance * instances_out, rtx_bvh_node * tlas_nodes_out,
                                 int32_t * tlas_indices_out, int32_t * tlas_node_count_out) {
    if (!tlas || instance_count <= 0 || !positions || !rotations || !blas_ids || !blas_root_aabbs || !instances_out || !tlas_nodes_out || !tlas_indices_out || !tlas_node_count_out)
        return RTX_ERR_INVALID_ARG;
    std::vector<float> aabbs(6 * (size_t)instance_count);
    for (int i = 0; i < instance_count; i++) {
        memset(&instances_out[i], 0, sizeof(rtx_instance));
        instances_out[i].blas_id = blas_ids[i];
        const float * box = blas_root_aabbs + 6 * (size_t)blas_ids[i];
        int rc = rtxh_instance_update(positions + 3 * i, rotations + 4 * i, box, box + 3, &instances_out[i], &aabbs[6 * (size_t)i], &aabbs[6 * (size_t)i + 3]);
        if (rc) return rc;
    }
    return rtxh_tlas_build(tlas, positions, aabbs.data(), tlas_nodes_out, tlas_indices_out, tlas_node_count_out);
}

extern "C" int rtxh_plane_update(const float position[3], const float rotation[4], int32_t material_id, rtx_plane * out) {
    if (!position || !rotation || !out) return RTX_ERR_INVALID_ARG;
    float w[16];
    world_matrix(position, rotation, w);                                     // Plane::update, Plane.cpp:3-11
    V n = m_direction(w, mk(0.0f, 1.0f, 0.0f));
    V p = mk(position[0], position[1], position[2]);
    float dist = -dot(n, p);
    V ua = m_direction(w, mk(1.0f, 0.0f, 0.0f));
    V va = cross(ua, n);
    memset(out, 0, sizeof(*out));
    out->normal[0] = n.x; out->normal[1] = n.y; out->normal[2] = n.z; out->distance = dist;
    out->u_axis[0] = ua.x; out->u_axis[1] = ua.y; out->u_axis[2] = ua.z;
    out->v_axis[0] = va.x; out->v_axis[1] = va.y; out->v_axis[2] = va.z;
    out->material_id = material_id;
    return RTX_OK;
}

// =================================================================================================
// TLAS: TopLevelBVH::init / build_bvh (TopLevelBVH.cpp:5-45) over BVHBuilders::build_bvh<Mesh>
// (BVHBuilders.h:8-46) and BVHPartitions::{calculate_bounds, partition_sah, split_indices}
// (BVHPartitions.h:10-114).  Same algorithm, same index-array persistence across frames, so the
// rebuilt tree is the reference's node for node (checked against dumped TLAS nodes in tests).
struct rtxh_tlas {
    int n;
    std::vector<int> idx[3];
    std::vector<float> sah;
    std::vector<int> temp;
};

namespace {
struct TlasBuild {        // BVHBuilders::build_bvh<PrimitiveType>: used for Mesh instances (TLAS) and for triangles (reference BLAS)
    const float * pos; const float * aabb; rtxh_tlas * t; rtx_bvh_node * nodes; int node_index;
    bool degenerate = false;     // NaN keys: the three sorted lists stop agreeing about who is left of the split (the reference overruns `temp` there)
    Box prim_box(int i) const { Box b; b.mn = mk(aabb[6 * i], aabb[6 * i + 1], aabb[6 * i + 2]); b.mx = mk(aabb[6 * i + 3], aabb[6 * i + 4], aabb[6 * i + 5]); return b; }
    float p(int i, int d) const { return pos[3 * i + d]; }

    void build(int node_id, int first, int count) {
        rtx_bvh_node & node = nodes[node_id];
        Box b = empty_box();                                            // calculate_bounds over indices[0]
        for (int i = first; i < first + count; i++) expand(b, prim_box(t->idx[0][i]));
        fix_if_needed(b);
        node.aabb_min[0] = b.mn.x; node.aabb_min[1] = b.mn.y; node.aabb_min[2] = b.mn.z;
        node.aabb_max[0] = b.mx.x; node.aabb_max[1] = b.mx.y; node.aabb_max[2] = b.mx.z;
        if (count < 3) { node.left_or_first = first; node.count = count; return; }
        const int left = node_index;
        node.left_or_first = left;
        node_index += 2;                                                // allocated before the SAH check, as the reference does

        // partition_sah: full sweep over the three sorted index lists
        float min_cost = INFINITY; int min_index = -1, min_dim = -1;
        for (int d = 0; d < 3; d++) {
            Box l = empty_box(), r = empty_box();
            for (int i = 0; i < count - 1; i++) { expand(l, prim_box(t->idx[d][first + i])); t->sah[i] = surface_area(l) * float(i + 1); }
            for (int i = count - 1; i > 0; i--) {
                expand(r, prim_box(t->idx[d][first + i]));
                float cost = t->sah[i - 1] + surface_area(r) * float(count - i);
                if (cost < min_cost) { min_cost = cost; min_index = first + i; min_dim = d; }
            }
        }
        float parent_cost = surface_area(b) * float(count);
        if (min_index < 0) { degenerate = true; node.left_or_first = first; node.count = count; return; }   // every cost NaN: nothing to split on
        if (min_cost >= parent_cost) { node.left_or_first = first; node.count = count; return; }

        // split_indices: keep the other two lists consistent with the chosen split
        const float split = p(t->idx[min_dim][min_index], min_dim);
        for (int d = 0; d < 3; d++) {
            if (d == min_dim) continue;
            int l = 0, r = min_index - first;
            for (int i = first; i < first + count; i++) {
                const int prim = t->idx[d][i];
                bool goes_left = p(prim, min_dim) < split;
                if (p(prim, min_dim) == split) {
                    int j = min_index - 1;
                    while (j >= first && p(t->idx[min_dim][j], min_dim) == split) {
                        if (t->idx[min_dim][j] == prim) { goes_left = true; break; }
                        j--;
                    }
                }
                if (goes_left) { if (l >= min_index - first) { degenerate = true; break; } t->temp[l++] = prim; }
                else           { if (r >= count)             { degenerate = true; break; } t->temp[r++] = prim; }
            }
            if (degenerate) { node.left_or_first = first; node.count = count; return; }
            memcpy(&t->idx[d][first], t->temp.data(), sizeof(int) * count);
        }
        node.count = (min_dim + 1) << 30;
        const int n_left = min_index - first, n_right = first + count - min_index;
        build(left, first, n_left);
        build(left + 1, first + n_left, n_right);
    }
};
}  // namespace

extern "C" int rtxh_tlas_create(int32_t n, rtxh_tlas ** out) {
    if (n <= 0 || !out) return RTX_ERR_INVALID_ARG;
    rtxh_tlas * t = new rtxh_tlas();
    t->n = n;
    for (int d = 0; d < 3; d++) { t->idx[d].resize(n); for (int i = 0; i < n; i++) t->idx[d][i] = i; }
    t->sah.resize(n); t->temp.resize(n);
    *out = t;
    return RTX_OK;
}
extern "C" int rtxh_tlas_destroy(rtxh_tlas * t) { if (!t) return RTX_ERR_INVALID_ARG; delete t; return RTX_OK; }

extern "C" int rtxh_tlas_build(rtxh_tlas * t, const float * positions, const float * aabbs,
                               rtx_bvh_node * nodes_out, int32_t * indices_out, int32_t * node_count_out) {
    if (!t || !positions || !aabbs || !nodes_out || !indices_out || !node_count_out) return RTX_ERR_INVALID_ARG;
    const int n = t->n;
    for (int d = 0; d < 3; d++)
        std::sort(t->idx[d].begin(), t->idx[d].end(), [&](int a, int b) { return positions[3 * a + d] < positions[3 * b + d]; });
    memset(nodes_out, 0, sizeof(rtx_bvh_node) * 2 * (size_t)n);
    TlasBuild b; b.pos = positions; b.aabb = aabbs; b.t = t; b.nodes = nodes_out; b.node_index = 2;
    b.build(0, 0, n);
    memcpy(indices_out, t->idx[0].data(), sizeof(int) * n);
    *node_count_out = b.node_index;
    return b.degenerate ? RTX_ERR_STATE : RTX_OK;
}

// ---- the balanced TLAS of rtx_update_instances: csrc/rtx_update_math.h, the code the kernels run, driven sequentially ----------------------
// the rigid rule of the length queries (rtxu::instance_rigid, csrc/rtx_update_math.h: the definition rtx_set_frame compiles)
extern "C" int rtxh_instances_rigid(const rtx_instance * instances, int32_t count, double * deviation_out) {
    bool rigid = true; double worst = 0.0;
    for (int32_t i = 0; instances && i < count; i++) {
        rigid = rigid && rtxu::instance_rigid(instances[i].world, instances[i].world_inv);
        const double a = rtxu::rigid_deviation(instances[i].world), b = rtxu::rigid_deviation(instances[i].world_inv);
        if (!(worst != worst)) worst = a != a || a > worst ? a : worst;      // a NaN stays
        if (!(worst != worst)) worst = b != b || b > worst ? b : worst;
    }
    if (deviation_out) *deviation_out = worst;
    return rigid ? 1 : 0;
}

extern "C" int32_t rtxh_tlas_balanced_node_count(int32_t n) { return n < 1 || n > RTX_UPDATE_MAX_INSTANCES ? 0 : rtxu::tree_node_count(n); }
extern "C" int32_t rtxh_tlas_balanced_inner_depth(int32_t n) { return rtxu::tree_inner_depth(n); }

extern "C" int rtxh_tlas_build_balanced(int32_t n, const float * positions, const float * aabbs,
                                        rtx_bvh_node * nodes_out, int32_t * indices_out, int32_t * node_count_out) {
    if (n < 1 || !positions || !aabbs || !nodes_out || !indices_out || !node_count_out) return RTX_ERR_INVALID_ARG;
    if (n > RTX_UPDATE_MAX_INSTANCES) return RTX_ERR_LIMIT;
    uint32_t bounds[6] = { RTXU_KEY_LO_INIT, RTXU_KEY_LO_INIT, RTXU_KEY_LO_INIT, RTXU_KEY_HI_INIT, RTXU_KEY_HI_INIT, RTXU_KEY_HI_INIT };
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            const float p = positions[3 * i + a];
            if (!rtxu::is_finite(p)) continue;
            const uint32_t k = rtxu::ordered_key(p);
            if (k < bounds[a]) bounds[a] = k;
            if (k > bounds[3 + a]) bounds[3 + a] = k;
        }
    std::vector<uint64_t> keys((size_t)n);
    for (int i = 0; i < n; i++) {
        rtxu::Box b; memcpy(b.mn, aabbs + 6 * (size_t)i, 12); memcpy(b.mx, aabbs + 6 * (size_t)i + 3, 12);
        keys[i] = rtxu::sort_key(positions + 3 * i, bounds, (uint32_t)i, rtxu::box_is_finite(b));
    }
    std::sort(keys.begin(), keys.end());                                // the keys are distinct (the index is part of them): one result
    const int levels = rtxu::tree_levels(n), slots = rtxu::tree_node_count(n);
    memset(nodes_out, 0, sizeof(rtx_bvh_node) * (size_t)slots);
    auto load = [&](int slot) { rtxu::Box b; memcpy(b.mn, nodes_out[slot].aabb_min, 12); memcpy(b.mx, nodes_out[slot].aabb_max, 12); return b; };
    auto store = [&](int slot, const rtxu::Box & b, int32_t left_or_first, int32_t count) {
        memcpy(nodes_out[slot].aabb_min, b.mn, 12); memcpy(nodes_out[slot].aabb_max, b.mx, 12);
        nodes_out[slot].left_or_first = left_or_first; nodes_out[slot].count = count;
    };
    for (int d = levels; d >= 0; d--)
        for (int j = 0; j < (1 << d); j++) {
            int first;
            const int cnt = rtxu::node_range(n, d, j, &first), slot = rtxu::node_slot(d, j);
            if (cnt == 0) continue;
            rtxu::Box b;
            if (cnt == 1) {
                const int inst = (int)(keys[first] & 0xffffu);
                indices_out[first] = inst;
                memcpy(b.mn, aabbs + 6 * (size_t)inst, 12); memcpy(b.mx, aabbs + 6 * (size_t)inst + 3, 12);
                rtxu::fix_if_needed(b);
                store(slot, b, first, 1);
            } else {
                const int left = (2 << d) | (2 * j);
                int axis;
                b = rtxu::join_boxes(load(left), load(left + 1), &axis);
                store(slot, b, left, (int32_t)((uint32_t)axis << 30));
            }
        }
    *node_count_out = slots;
    return RTX_OK;
}

extern "C" int rtxh_scene_update_balanced(int32_t n, const float * positions, const float * rotations, const int32_t * blas_ids,
                                          const float * blas_root_aabbs, rtx_instance * instances_out, rtx_bvh_node * tlas_nodes_out,
                                          int32_t * tlas_indices_out, int32_t * tlas_node_count_out) {
    if (n < 1 || !positions || !rotations || !blas_ids || !blas_root_aabbs || !instances_out || !tlas_nodes_out || !tlas_indices_out || !tlas_node_count_out)
        return RTX_ERR_INVALID_ARG;
    if (n > RTX_UPDATE_MAX_INSTANCES) return RTX_ERR_LIMIT;
    std::vector<float> aabbs(6 * (size_t)n);
    for (int i = 0; i < n; i++) {
        memset(&instances_out[i], 0, sizeof(rtx_instance));
        instances_out[i].blas_id = blas_ids[i];
        const float * box = blas_root_aabbs + 6 * (size_t)blas_ids[i];
        rtxu::world_matrix(positions + 3 * i, rotations + 4 * i, instances_out[i].world);
        rtxu::invert(instances_out[i].world, instances_out[i].world_inv);
        const rtxu::Box b = rtxu::transform_box(instances_out[i].world, box, box + 3);
        memcpy(&aabbs[6 * (size_t)i], b.mn, 12); memcpy(&aabbs[6 * (size_t)i + 3], b.mx, 12);
    }
    return rtxh_tlas_build_balanced(n, positions, aabbs.data(), tlas_nodes_out, tlas_indices_out, tlas_node_count_out);
}

// The reference's non-spatial BLAS build (BottomLevelBVH::build_bvh, BottomLevelBVH.cpp:72-106): the same generic builder
// over triangles, keyed by Triangle::get_position (Triangle.h:22-24) with AABBs from Triangle::calc_aabb (:14-20).
extern "C" int rtxh_blas_build_reference_bvh(const float * positions, int32_t n, rtx_bvh_node * nodes_out, int32_t * node_count_out, int32_t * order_out) {
    if (!positions || n <= 0 || !nodes_out || !node_count_out || !order_out) return RTX_ERR_INVALID_ARG;
    std::vector<float> cen(3 * (size_t)n), box(6 * (size_t)n);
    for (int i = 0; i < n; i++) {
        const float * p = positions + 9 * (size_t)i;
        V a = mk(p[0], p[1], p[2]), b = mk(p[3], p[4], p[5]), c = mk(p[6], p[7], p[8]);
        Box t = empty_box(); expand(t, a); expand(t, b); expand(t, c);
        fix_if_needed(t); fix_if_needed(t);                                   // AABB::from_points, then calc_aabb's own call
        V g = (a + b + c) * (1.0f / 3.0f);
        cen[3 * (size_t)i] = g.x; cen[3 * (size_t)i + 1] = g.y; cen[3 * (size_t)i + 2] = g.z;
        box[6 * (size_t)i] = t.mn.x; box[6 * (size_t)i + 1] = t.mn.y; box[6 * (size_t)i + 2] = t.mn.z;
        box[6 * (size_t)i + 3] = t.mx.x; box[6 * (size_t)i + 4] = t.mx.y; box[6 * (size_t)i + 5] = t.mx.z;
    }
    rtxh_tlas * t = nullptr;
    int rc = rtxh_tlas_create(n, &t);
    if (rc) return rc;
    rc = rtxh_tlas_build(t, cen.data(), box.data(), nodes_out, order_out, node_count_out);
    rtxh_tlas_destroy(t);
    return rc;
}

// =================================================================================================
// BLAS: this repo's own builder — top-down binned SAH over triangle centroids.  Output follows the
// conventions the traversal relies on (BVHNode.h:10-28): root 0, index 1 unused, children adjacent,
// split axis in the top two bits of `count`, leaves index a flattened triangle order.
namespace {
struct BlasBuild {
    const float * pos; int bins;
    std::vector<Box> tb; std::vector<V> cen; std::vector<int> order;
    rtx_bvh_node * nodes; int node_index;

    void set_box(rtx_bvh_node & n, Box b) {
        fix_if_needed(b);
        n.aabb_min[0] = b.mn.x; n.aabb_min[1] = b.mn.y; n.aabb_min[2] = b.mn.z;
        n.aabb_max[0] = b.mx.x; n.aabb_max[1] = b.mx.y; n.aabb_max[2] = b.mx.z;
    }

    void build(int node_id, int first, int count) {
        Box b = empty_box(), cb = empty_box();
        for (int i = first; i < first + count; i++) { expand(b, tb[order[i]]); expand(cb, cen[order[i]]); }
        set_box(nodes[node_id], b);
        if (count < 3) { nodes[node_id].left_or_first = first; nodes[node_id].count = count; return; }

        float best_cost = INFINITY; int best_dim = -1, best_bin = -1;
        const int NB = bins;
        std::vector<Box> bb(NB); std::vector<int> bc(NB);
        std::vector<float> right_sa(NB);
        for (int d = 0; d < 3; d++) {
            const float lo = comp(cb.mn, d), hi = comp(cb.mx, d);
            if (!(hi > lo)) continue;
            const float scale = float(NB) / (hi - lo);
            for (int k = 0; k < NB; k++) { bb[k] = empty_box(); bc[k] = 0; }
            for (int i = first; i < first + count; i++) {
                int k = (int)((comp(cen[order[i]], d) - lo) * scale); if (k >= NB) k = NB - 1; if (k < 0) k = 0;
                expand(bb[k], tb[order[i]]); bc[k]++;
            }
            Box r = empty_box(); int rc = 0;
            for (int k = NB - 1; k > 0; k--) { if (bc[k]) expand(r, bb[k]); rc += bc[k]; right_sa[k] = rc ? surface_area(r) * float(rc) : 0.0f; }
            Box l = empty_box(); int lc = 0;
            for (int k = 0; k < NB - 1; k++) {
                if (bc[k]) expand(l, bb[k]); lc += bc[k];
                if (lc == 0 || lc == count) continue;
                const float cost = surface_area(l) * float(lc) + right_sa[k + 1];
                if (cost < best_cost) { best_cost = cost; best_dim = d; best_bin = k; }
            }
        }
        Box fb = b; fix_if_needed(fb);
        const float parent_cost = surface_area(fb) * float(count);
        int mid;
        if (best_dim < 0 || best_cost >= parent_cost) {
            if (count <= 4) { nodes[node_id].left_or_first = first; nodes[node_id].count = count; return; }
            // no useful SAH split for a large set (coincident centroids): split the index range in half
            best_dim = 0; { V e = cb.mx - cb.mn; if (e.y > e.x) best_dim = 1; if (e.z > comp(e, best_dim)) best_dim = 2; }
            mid = first + count / 2;
            std::nth_element(order.begin() + first, order.begin() + mid, order.begin() + first + count,
                             [&](int a, int c) { return comp(cen[a], best_dim) < comp(cen[c], best_dim); });
        } else {
            const float lo = comp(cb.mn, best_dim), hi = comp(cb.mx, best_dim);
            const float scale = float(NB) / (hi - lo);
            int * beg = order.data() + first;
            int * m = std::partition(beg, beg + count, [&](int a) {
                int k = (int)((comp(cen[a], best_dim) - lo) * scale); if (k >= NB) k = NB - 1; if (k < 0) k = 0;
                return k <= best_bin; });
            mid = (int)(m - order.data());
        }
        const int left = node_index; node_index += 2;
        nodes[node_id].left_or_first = left;
        nodes[node_id].count = (best_dim + 1) << 30;
        build(left, first, mid - first);
        build(left + 1, mid, first + count - mid);
    }
};
}  // namespace

extern "C" int rtxh_blas_build(const float * positions, int32_t n, int32_t bins, rtx_bvh_node * nodes_out, int32_t * node_count_out, int32_t * order_out) {
    if (!positions || n <= 0 || !nodes_out || !node_count_out || !order_out) return RTX_ERR_INVALID_ARG;
    if (bins < 4) bins = 4;
    if (bins > 256) bins = 256;
    BlasBuild b; b.pos = positions; b.bins = bins; b.tb.resize(n); b.cen.resize(n); b.order.resize(n);
    for (int i = 0; i < n; i++) {
        const float * p = positions + 9 * (size_t)i;
        Box t = empty_box();
        expand(t, mk(p[0], p[1], p[2])); expand(t, mk(p[3], p[4], p[5])); expand(t, mk(p[6], p[7], p[8]));
        b.cen[i] = 0.5f * (t.mn + t.mx);
        fix_if_needed(t);
        b.tb[i] = t; b.order[i] = i;
    }
    memset(nodes_out, 0, sizeof(rtx_bvh_node) * 2 * (size_t)n);
    b.nodes = nodes_out; b.node_index = 2;
    b.build(0, 0, n);
    memcpy(order_out, b.order.data(), sizeof(int) * n);
    *node_count_out = b.node_index;
    return RTX_OK;
}

// =================================================================================================
// Texture::load mip chain, Texture.cpp:76-117 (box filter, levels appended after level 0)
extern "C" int rtxh_texture_mips(float * tx, int32_t width, int32_t height, rtx_texture_desc * desc, int64_t * texel_count_out) {
    if (!tx || !desc || width <= 0 || height <= 0) return RTX_ERR_INVALID_ARG;
    int64_t count = 0;
    if (int rc = rtxt::chain_shape(width, height, 1, desc, &count)) return rc;      // the shape and the filter the device chain has too (rtx_texmip_math.h)
    for (int l = 1; l < desc->mip_levels; l++) {
        const int lw = width >> l, lh = height >> l, lwp = width >> (l - 1);
        const float * prev = tx + 3 * (size_t)desc->mip_offsets[l - 1];
        float * o = tx + 3 * (size_t)desc->mip_offsets[l];
        for (int j = 0; j < lh; j++) for (int i = 0; i < lw; i++, o += 3) {
            const float * c0 = prev + 3 * ((size_t)(2 * i) + (size_t)(2 * j) * lwp), * c2 = c0 + 3 * (size_t)lwp;
            for (int k = 0; k < 3; k++) o[k] = rtxt::box(c0[k], c0[3 + k], c2[k], c2[3 + k]);
        }
    }
    if (texel_count_out) *texel_count_out = count;
    return RTX_OK;
}

// =================================================================================================
// RTX_QUERY_SORT on the host: the round structure of rtx_query_closest / rtx_query_occluded, the bounds as the twelve min-reduced words
// k_query_sort_bounds leaves, the keys of rtx_query_sort_math.h, a sort of the 64-bit keys (a total order: any sort gives this result)
extern "C" int rtxh_query_sort_order(const float * rows, int32_t row_floats, int64_t n, int32_t * order_out) {
    if (!rows || !order_out || n < 1 || (row_floats != 4 && row_floats != 6 && row_floats != 7)) return RTX_ERR_INVALID_ARG;
    if (n > (int64_t)INT32_MAX) return RTX_ERR_LIMIT;
    std::vector<uint64_t> keys;
    for (int64_t first = 0; first < n; first += RTX_QUERY_CHUNK_RAYS) {
        const int m = (int)(n - first < (int64_t)RTX_QUERY_CHUNK_RAYS ? n - first : (int64_t)RTX_QUERY_CHUNK_RAYS);
        const float * const r = rows + (size_t)row_floats * first;
        uint32_t bounds[2 * rtxq::COORDS];
        for (uint32_t & b : bounds) b = 0xffffffffu;
        for (int i = 0; i < m; i++) {
            if (!rtxq::row_is_live(r + (size_t)row_floats * i, row_floats)) continue;
            float x[rtxq::COORDS]; uint32_t k12[2 * rtxq::COORDS];
            rtxq::coordinates(r + (size_t)row_floats * i, row_floats, x);
            rtxq::bounds_of_row(x, k12);
            for (int a = 0; a < 2 * rtxq::COORDS; a++) if (k12[a] < bounds[a]) bounds[a] = k12[a];
        }
        const rtxq::Plan plan = rtxq::make_plan(bounds);
        keys.resize((size_t)m);
        for (int i = 0; i < m; i++) keys[i] = rtxq::sort_key(plan, r + (size_t)row_floats * i, row_floats, (uint32_t)i);
        std::sort(keys.begin(), keys.end());
        for (int i = 0; i < m; i++) order_out[first + i] = (int32_t)first + (int32_t)rtxq::key_row(keys[i]);
    }
    return RTX_OK;
}

// =================================================================================================
// rtx_query_nearest on the host: rtxnp::walk (csrc/rtx_nearest_math.h) over the reference-layout arrays, and the exhaustive search
namespace {
struct HostNearestScene {
    const rtxh_nearest_scene & s;
    const rtxh_nearest_blas * B = nullptr;
    RTX_WALK_UNFILTERED
    int sphere_count() const { return s.sphere_count; }
    int plane_count() const { return s.plane_count; }
    int tlas_nodes() const { return s.tlas_node_count; }
    void sphere(int i, rtxnp::P3 & c, float & r2) const { c = rtxnp::ptr3(s.spheres[i].center); r2 = s.spheres[i].radius_squared; }
    void plane(int i, rtxnp::P3 & n, float & dist) const { n = rtxnp::ptr3(s.planes[i].normal); dist = s.planes[i].distance; }
    static void node(const rtx_bvh_node & nd, rtxnp::P3 & mn, rtxnp::P3 & mx, int & first, int & count) {
        mn = rtxnp::ptr3(nd.aabb_min); mx = rtxnp::ptr3(nd.aabb_max); first = nd.left_or_first; count = nd.count;
    }
    void tlas_node(int i, rtxnp::P3 & mn, rtxnp::P3 & mx, int & first, int & count) const { node(s.tlas_nodes[i], mn, mx, first, count); }
    void blas_node(int i, rtxnp::P3 & mn, rtxnp::P3 & mx, int & first, int & count) const { node(B->nodes[i], mn, mx, first, count); }
    int enter(int slot, rtxnp::P3 p, rtxnp::P3 & pl) {
        const int inst = s.tlas_indices[slot];
        pl = rtxnp::xform_pos(s.instances[inst].world_inv, p);
        B = &s.blas[s.instances[inst].blas_id];
        return inst;
    }
    void triangle(int i, rtxnp::P3 & p0, rtxnp::P3 & e1, rtxnp::P3 & e2) const {
        p0 = rtxnp::ptr3(B->hot[i].position_0); e1 = rtxnp::ptr3(B->hot[i].position_edge_1); e2 = rtxnp::ptr3(B->hot[i].position_edge_2);
    }
};
// FILTER of rtx_nearest_math.h over plain arrays: table = M object masks (null: all ones), row_mask = the row's
struct HostMasks {
    const uint32_t * table; const uint32_t * rows; uint32_t row;
    uint32_t of_row(int64_t i) const { return rows ? rows[i] : row; }
};
template <typename Base> struct HostMasked : Base {
    const uint32_t * table; uint32_t row_mask;
    HostMasked(const rtxh_nearest_scene & sc, const uint32_t * table_, uint32_t row_mask_) : Base{ sc }, table(table_), row_mask(row_mask_) {}
    bool row_visible() const { return row_mask != 0u; }
    bool object_visible(int object) const { return !table || rtxnp::mask_visible(table[object], row_mask); }
    bool sphere_visible(int i) const { return object_visible(this->s.instance_count + i); }
    bool plane_visible(int i) const { return object_visible(this->s.instance_count + this->s.sphere_count + i); }
    bool instance_visible(int slot) const { return object_visible(this->s.tlas_indices[slot]); }
};
struct HostNearestStack {
    int node[RTX_MAX_STACK]; float d2[RTX_MAX_STACK]; int high = 0;
    void push(int sp, int n, float d) { node[sp] = n; d2[sp] = d; if (sp + 1 > high) high = sp + 1; }
    void pop(int sp, int & n, float & d) const { n = node[sp]; d = d2[sp]; }
};
int tree_inner_depth(const rtx_bvh_node * nodes, int node_count, int64_t primitive_count, int & depth_out) {      // -1: one leaf; error: a child or a range outside its array
    depth_out = -1;
    if (node_count < 1) return RTX_ERR_INVALID_ARG;
    std::vector<std::pair<int, int>> todo(1, std::make_pair(0, 0));
    size_t visited = 0;
    while (!todo.empty()) {
        const int i = todo.back().first, d = todo.back().second; todo.pop_back();
        if (++visited > (size_t)node_count) return RTX_ERR_INVALID_ARG;      // a cycle
        const int cnt = nodes[i].count & 0x3fffffff, f = nodes[i].left_or_first;
        if (cnt > 0) { if (f < 0 || (int64_t)f + cnt > primitive_count) return RTX_ERR_INVALID_ARG; }
        else { if (f < 0 || f + 1 >= node_count) return RTX_ERR_INVALID_ARG; if (d > depth_out) depth_out = d; todo.push_back(std::make_pair(f, d + 1)); todo.push_back(std::make_pair(f + 1, d + 1)); }
    }
    return RTX_OK;
}
int nearest_scene_check(const rtxh_nearest_scene * s, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out, bool trees, bool may_be_empty = false) {
    if (!s || !points || n < 1 || (channels & ~(uint32_t)RTX_QUERY_ALL)) return RTX_ERR_INVALID_ARG;
    if (may_be_empty ? (channels != 0 && !out) : (!out || channels == 0)) return RTX_ERR_INVALID_ARG;      // a signed query may ask for no channel
    if (s->instance_count < 0 || s->tlas_node_count < 0 || s->tlas_index_count < 0 || s->blas_count < 0 || s->sphere_count < 0 || s->plane_count < 0) return RTX_ERR_INVALID_ARG;
    if ((s->instance_count && !s->instances) || (s->tlas_node_count && !s->tlas_nodes) || (s->tlas_index_count && !s->tlas_indices) || (s->blas_count && !s->blas) ||
        (s->sphere_count && !s->spheres) || (s->plane_count && !s->planes)) return RTX_ERR_INVALID_ARG;
    for (int i = 0; i < s->instance_count; i++) if (s->instances[i].blas_id < 0 || s->instances[i].blas_id >= s->blas_count) return RTX_ERR_INVALID_ARG;
    for (int b = 0; b < s->blas_count; b++) if (!s->blas[b].nodes || !s->blas[b].hot || !s->blas[b].cold || s->blas[b].node_count < 1 || s->blas[b].triangle_count < 0) return RTX_ERR_INVALID_ARG;
    for (int i = 0; i < s->tlas_index_count; i++) if (s->tlas_indices[i] < 0 || s->tlas_indices[i] >= s->instance_count) return RTX_ERR_INVALID_ARG;
    if (!trees) return RTX_OK;
    int tlas_depth = -1, blas_depth = -1;
    if (s->tlas_node_count > 0) if (int rc = tree_inner_depth(s->tlas_nodes, s->tlas_node_count, s->tlas_index_count, tlas_depth)) return rc;
    for (int b = 0; b < s->blas_count; b++) {
        int d = -1;
        if (int rc = tree_inner_depth(s->blas[b].nodes, s->blas[b].node_count, s->blas[b].triangle_count, d)) return rc;
        if (d > blas_depth) blas_depth = d;
    }
    return rtxnp::stack_need(tlas_depth, blas_depth) > RTX_MAX_STACK ? RTX_ERR_LIMIT : RTX_OK;
}
// the channels of row i from its answer: what k_query_nearest stores
void nearest_store(const rtxh_nearest_scene & s, const float * row, const rtxnp::Answer & a, int64_t i, uint32_t channels, const rtx_query_buffers & out) {
    const bool hit = a.kind != rtxnp::KIND_NONE;
    rtxnp::P3 point = rtxnp::mk(0.0f, 0.0f, 0.0f), normal = point;
    float tu = 0.0f, tv = 0.0f; int material = -1;
    const rtxnp::P3 p = rtxnp::mk(row[0], row[1], row[2]);
    if (a.kind == rtxnp::KIND_TRI) {
        const rtx_instance & I = s.instances[a.object];
        const rtxh_nearest_blas & B = s.blas[I.blas_id];
        const rtx_triangle_hot & h = B.hot[a.slot]; const rtx_triangle_cold & c = B.cold[a.slot];
        point = rtxnp::xform_pos(I.world, rtxnp::triangle_point(rtxnp::ptr3(h.position_0), rtxnp::ptr3(h.position_edge_1), rtxnp::ptr3(h.position_edge_2), a.u, a.v));
        rtxnp::triangle_outputs(I.world, rtxnp::ptr3(c.normal_0), rtxnp::ptr3(c.normal_edge_1), rtxnp::ptr3(c.normal_edge_2), c.tex_coord_0, c.tex_coord_edge_1, c.tex_coord_edge_2, a.u, a.v, normal, tu, tv);
        material = B.material_offset + c.material_id;
    } else if (a.kind == rtxnp::KIND_SPHERE) {
        const rtx_sphere & sp = s.spheres[a.object];
        rtxnp::sphere_outputs(p, rtxnp::ptr3(sp.center), sp.radius_squared, point, normal, tu, tv); material = sp.material_id;
    } else if (a.kind == rtxnp::KIND_PLANE) {
        const rtx_plane & pl = s.planes[a.object];
        rtxnp::plane_outputs(p, rtxnp::ptr3(pl.normal), pl.distance, rtxnp::ptr3(pl.u_axis), rtxnp::ptr3(pl.v_axis), point, normal, tu, tv); material = pl.material_id;
    }
    auto on = [&](uint32_t bit) { return (channels & bit) != 0; };
    if (on(RTX_QUERY_DISTANCE) && out.distance) out.distance[i] = hit ? rtxnp::root(a.d2) : INFINITY;
    if (on(RTX_QUERY_POSITION) && out.position) { out.position[3 * i] = point.x; out.position[3 * i + 1] = point.y; out.position[3 * i + 2] = point.z; }
    if (on(RTX_QUERY_NORMAL) && out.normal) { out.normal[3 * i] = normal.x; out.normal[3 * i + 1] = normal.y; out.normal[3 * i + 2] = normal.z; }
    if (on(RTX_QUERY_UV) && out.uv) { out.uv[2 * i] = tu; out.uv[2 * i + 1] = tv; }
    if (on(RTX_QUERY_MATERIAL_ID) && out.material_id) out.material_id[i] = hit ? material : -1;
    if (on(RTX_QUERY_OBJECT_ID) && out.object_id)
        out.object_id[i] = !hit ? -1 : a.kind == rtxnp::KIND_TRI ? a.object : a.kind == rtxnp::KIND_SPHERE ? s.instance_count + a.object : s.instance_count + s.sphere_count + a.object;
    if (on(RTX_QUERY_TRIANGLE_ID) && out.triangle_id) out.triangle_id[i] = a.kind == rtxnp::KIND_TRI ? a.slot : -1;
}
// SIDE of csrc/rtx_side_math.h over plain arrays: the tables of one mesh (null: none), and what k_query_nearest<.., SIGNED> stores for row i
struct HostSideTables {
    const rtxh_side_blas * t;
    bool has_tables() const { return t && t->vert_pn && t->edge_pn && t->slot_vertices; }
    rtxnp::P3 edge(int i) const { return rtxnp::ptr3(t->edge_pn + 4 * (size_t)i); }
    rtxnp::P3 vertex(int slot, int k) const {
        const int32_t v = t->slot_vertices[3 * (size_t)slot + k];
        return v < 0 || v >= t->vertex_count ? rtxnp::mk(0.0f, 0.0f, 0.0f) : rtxnp::ptr3(t->vert_pn + 4 * (size_t)v);
    }
};
struct HostSigned { const rtxh_side_blas * side; float * signed_out; int32_t * feature_out; };
void signed_store(const rtxh_nearest_scene & s, const float * row, const rtxnp::Answer & a, int64_t i, const HostSigned & sg) {
    const rtxnp::P3 p = rtxnp::mk(row[0], row[1], row[2]);
    bool negative = false; int feature = rtxsd::FEATURE_NONE;
    if (a.kind == rtxnp::KIND_TRI) {
        const rtx_instance & I = s.instances[a.object];
        const rtx_triangle_hot & h = s.blas[I.blas_id].hot[a.slot];
        const HostSideTables tb = { sg.side ? sg.side + I.blas_id : nullptr };
        feature = rtxsd::triangle_side(rtxnp::sub(rtxnp::xform_pos(I.world_inv, p), rtxnp::ptr3(h.position_0)), rtxnp::ptr3(h.position_edge_1), rtxnp::ptr3(h.position_edge_2), a.slot, tb, negative);
    } else if (a.kind == rtxnp::KIND_SPHERE) { negative = rtxsd::sphere_side(p, rtxnp::ptr3(s.spheres[a.object].center), s.spheres[a.object].radius_squared); feature = rtxsd::FEATURE_SPHERE; }
    else if (a.kind == rtxnp::KIND_PLANE) { negative = rtxsd::plane_side(p, rtxnp::ptr3(s.planes[a.object].normal), s.planes[a.object].distance); feature = rtxsd::FEATURE_PLANE; }
    sg.signed_out[i] = a.kind != rtxnp::KIND_NONE ? rtxsd::signed_distance(a.d2, negative) : INFINITY;
    if (sg.feature_out) sg.feature_out[i] = feature;
}
const rtx_query_buffers kNoBuffers = {};
// what the walk twins of the length queries refuse with RTX_ERR_STATE, as the device calls do (the exhaustive searches prune nothing and answer)
bool scene_rigid(const rtxh_nearest_scene & s) { return rtxh_instances_rigid(s.instances, s.instance_count, nullptr) == 1; }
}  // namespace

static int query_nearest_host(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out, int32_t * stack_max_out, const HostMasks * km,
                              const HostSigned * sg = nullptr) {
    if (sg && !sg->signed_out) return RTX_ERR_INVALID_ARG;
    if (int rc = nearest_scene_check(scene, points, n, channels, out, true, sg != nullptr)) return rc;
    if (!scene_rigid(*scene)) return RTX_ERR_STATE;
    if (!out) out = &kNoBuffers;
    int high = 0;
    for (int64_t i = 0; i < n; i++) {
        HostNearestStack st;
        rtxnp::Answer a;
        if (km) { HostMasked<HostNearestScene> S(*scene, km->table, km->of_row(i)); rtxnp::walk(S, st, points + 4 * i, a); }
        else { HostNearestScene S{ *scene }; rtxnp::walk(S, st, points + 4 * i, a); }
        if (st.high > high) high = st.high;
        nearest_store(*scene, points + 4 * i, a, i, channels, *out);
        if (sg) signed_store(*scene, points + 4 * i, a, i, *sg);
    }
    if (stack_max_out) *stack_max_out = high;
    return RTX_OK;
}

extern "C" int rtxh_query_nearest(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out, int32_t * stack_max_out) {
    return query_nearest_host(scene, points, n, channels, out, stack_max_out, nullptr);
}
extern "C" int rtxh_query_nearest_filtered(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out, int32_t * stack_max_out,
                                           const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_nearest_host(scene, points, n, channels, out, stack_max_out, &km);
}

static int query_nearest_exhaustive_host(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out, const HostMasks km,
                                         const HostSigned * sg = nullptr) {
    if (sg && !sg->signed_out) return RTX_ERR_INVALID_ARG;
    if (int rc = nearest_scene_check(scene, points, n, channels, out, false, sg != nullptr)) return rc;
    if (!out) out = &kNoBuffers;
    const rtxh_nearest_scene & s = *scene;
    for (int64_t i = 0; i < n; i++) {
        const float * row = points + 4 * i;
        const HostMasked<HostNearestScene> vis(s, km.table, km.of_row(i));
        rtxnp::Answer a; a.kind = rtxnp::KIND_NONE; a.object = -1; a.slot = -1; a.u = 0.0f; a.v = 0.0f; a.d2 = INFINITY;
        if (rtxnp::row_is_live(row) && vis.row_visible()) {
            const rtxnp::P3 p = rtxnp::mk(row[0], row[1], row[2]);
            a.d2 = row[3] * row[3];
            for (int k = 0; k < s.sphere_count; k++) if (vis.sphere_visible(k)) rtxnp::offer(a, rtxnp::sphere_d2(p, rtxnp::ptr3(s.spheres[k].center), s.spheres[k].radius_squared), rtxnp::KIND_SPHERE, k, -1, 0.0f, 0.0f);
            for (int k = 0; k < s.plane_count; k++) if (vis.plane_visible(k)) rtxnp::offer(a, rtxnp::plane_d2(p, rtxnp::ptr3(s.planes[k].normal), s.planes[k].distance), rtxnp::KIND_PLANE, k, -1, 0.0f, 0.0f);
            for (int k = 0; k < s.instance_count; k++) {
                if (!vis.object_visible(k)) continue;
                const rtxnp::P3 pl = rtxnp::xform_pos(s.instances[k].world_inv, p);
                const rtxh_nearest_blas & B = s.blas[s.instances[k].blas_id];
                for (int t = 0; t < B.triangle_count; t++) {
                    float u, v;
                    const float d2 = rtxnp::triangle_d2(rtxnp::sub(pl, rtxnp::ptr3(B.hot[t].position_0)), rtxnp::ptr3(B.hot[t].position_edge_1), rtxnp::ptr3(B.hot[t].position_edge_2), u, v);
                    rtxnp::offer(a, d2, rtxnp::KIND_TRI, k, t, u, v);
                }
            }
        }
        nearest_store(s, row, a, i, channels, *out);
        if (sg) signed_store(s, row, a, i, *sg);
    }
    return RTX_OK;
}
static const HostMasks kNoMasks = { nullptr, nullptr, 0xffffffffu };      // every object, every row: the unfiltered exhaustive searches
extern "C" int rtxh_query_nearest_exhaustive(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out) {
    return query_nearest_exhaustive_host(scene, points, n, channels, out, kNoMasks);
}
extern "C" int rtxh_query_nearest_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                                      const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_nearest_exhaustive_host(scene, points, n, channels, out, km);
}

// rtx_query_signed_distance on the host: the nearest-point searches above, then SIDE of csrc/rtx_side_math.h for the winner
extern "C" int rtxh_query_signed_distance(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                          const rtxh_side_blas * side, float * signed_out, int32_t * feature_out, int32_t * stack_max_out) {
    const HostSigned sg = { side, signed_out, feature_out };
    return query_nearest_host(scene, points, n, channels, out, stack_max_out, nullptr, &sg);
}
extern "C" int rtxh_query_signed_distance_filtered(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                                   const rtxh_side_blas * side, float * signed_out, int32_t * feature_out, int32_t * stack_max_out,
                                                   const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostSigned sg = { side, signed_out, feature_out };
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_nearest_host(scene, points, n, channels, out, stack_max_out, &km, &sg);
}
extern "C" int rtxh_query_signed_distance_exhaustive(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                                     const rtxh_side_blas * side, float * signed_out, int32_t * feature_out) {
    const HostSigned sg = { side, signed_out, feature_out };
    return query_nearest_exhaustive_host(scene, points, n, channels, out, kNoMasks, &sg);
}
extern "C" int rtxh_query_signed_distance_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                                              const rtxh_side_blas * side, float * signed_out, int32_t * feature_out,
                                                              const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostSigned sg = { side, signed_out, feature_out };
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_nearest_exhaustive_host(scene, points, n, channels, out, km, &sg);
}

extern "C" float rtxh_nearest_distance_bound(float local_scale, float world_scale) { return rtxnp::distance_bound(local_scale, world_scale); }
extern "C" float rtxh_nearest_box_d2(const float p[3], const float box_min[3], const float box_max[3]) { return rtxnp::box_d2(rtxnp::ptr3(p), rtxnp::ptr3(box_min), rtxnp::ptr3(box_max)); }
extern "C" float rtxh_nearest_triangle_d2(const float p[3], const rtx_triangle_hot * tri, float uv_out[2]) {
    float u, v;
    const float d2 = rtxnp::triangle_d2(rtxnp::sub(rtxnp::ptr3(p), rtxnp::ptr3(tri->position_0)), rtxnp::ptr3(tri->position_edge_1), rtxnp::ptr3(tri->position_edge_2), u, v);
    if (uv_out) { uv_out[0] = u; uv_out[1] = v; }
    return d2;
}
extern "C" float rtxh_nearest_sphere_d2(const float p[3], const rtx_sphere * sphere) { return rtxnp::sphere_d2(rtxnp::ptr3(p), rtxnp::ptr3(sphere->center), sphere->radius_squared); }
extern "C" float rtxh_nearest_plane_d2(const float p[3], const rtx_plane * plane) { return rtxnp::plane_d2(rtxnp::ptr3(p), rtxnp::ptr3(plane->normal), plane->distance); }

// =================================================================================================
// rtx_query_hits on the host: rtxhp::walk (csrc/rtx_hits_math.h) over the arrays of rtxh_query_nearest, and the exhaustive search
namespace {
struct HostHitsScene : HostNearestScene {
    explicit HostHitsScene(const rtxh_nearest_scene & sc) : HostNearestScene{ sc } {}
    int instance_count() const { return s.instance_count; }
    int enter(int slot, rtxnp::P3 o, rtxnp::P3 d, rtxnp::P3 & co, rtxnp::P3 & cd) {
        const int inst = s.tlas_indices[slot];
        co = rtxnp::xform_pos(s.instances[inst].world_inv, o);
        cd = rtxnp::xform_dir(s.instances[inst].world_inv, d);
        B = &s.blas[s.instances[inst].blas_id];
        return inst;
    }
};
struct HostHitsList {
    float t[rtxhp::MAX_HITS]; int32_t object[rtxhp::MAX_HITS], triangle[rtxhp::MAX_HITS];
    void get(int j, float & t_, int32_t & o_, int32_t & s_) const { t_ = t[j]; o_ = object[j]; s_ = triangle[j]; }
    void set(int j, float t_, int32_t o_, int32_t s_) { t[j] = t_; object[j] = o_; triangle[j] = s_; }
};
int hits_args_check(const rtxh_nearest_scene * s, const float * segments, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out, const int32_t * count_out, bool trees) {
    const bool count_only = max_hits == 0 && channels == 0 && count_out;
    if (!count_only && (max_hits < 1 || max_hits > rtxhp::MAX_HITS || channels == 0 || (channels & ~(uint32_t)RTX_QUERY_ALL) || !out)) return RTX_ERR_INVALID_ARG;
    const rtx_query_buffers none = {};
    return nearest_scene_check(s, segments, n, count_only ? (uint32_t)RTX_QUERY_DISTANCE : channels, count_only ? &none : out, trees);
}
// the channels of the K entries of row i from its list: what k_query_hits stores
void hit_write(const rtxh_nearest_scene & s, const float * row, const HostHitsList & L, int held, int K, int64_t i, uint32_t channels, const rtx_query_buffers & out) {
    auto on = [&](uint32_t bit) { return (channels & bit) != 0; };
    const rtxnp::P3 o = rtxnp::mk(row[0], row[1], row[2]), d = rtxnp::mk(row[3], row[4], row[5]);
    for (int j = 0; j < K; j++) {
        const size_t e = (size_t)i * (size_t)K + (size_t)j;
        const bool hit = j < held;
        rtxnp::P3 point = rtxnp::mk(0.0f, 0.0f, 0.0f), normal = point;
        float tu = 0.0f, tv = 0.0f; int material = -1;
        const float t = hit ? L.t[j] : INFINITY;
        const int32_t object = hit ? L.object[j] : -1, triangle = hit ? L.triangle[j] : -1;
        if (hit && triangle >= 0) {
            const rtx_instance & I = s.instances[object];
            const rtxh_nearest_blas & B = s.blas[I.blas_id];
            const rtx_triangle_hot & h = B.hot[triangle]; const rtx_triangle_cold & c = B.cold[triangle];
            const rtxnp::P3 co = rtxnp::xform_pos(I.world_inv, o), cd = rtxnp::xform_dir(I.world_inv, d);
            point = rtxnp::xform_pos(I.world, rtxhp::point_at(co, cd, t));
            float t2, u = 0.0f, v = 0.0f;
            rtxhp::tri_test(rtxnp::ptr3(h.position_0), rtxnp::ptr3(h.position_edge_1), rtxnp::ptr3(h.position_edge_2), co, cd, row[6], t2, u, v);
            rtxnp::triangle_outputs(I.world, rtxnp::ptr3(c.normal_0), rtxnp::ptr3(c.normal_edge_1), rtxnp::ptr3(c.normal_edge_2), c.tex_coord_0, c.tex_coord_edge_1, c.tex_coord_edge_2, u, v, normal, tu, tv);
            material = B.material_offset + c.material_id;
        } else if (hit && object < s.instance_count + s.sphere_count) {
            const rtx_sphere & sp = s.spheres[object - s.instance_count];
            rtxhp::sphere_outputs(o, d, t, rtxnp::ptr3(sp.center), sp.radius_inv, point, normal, tu, tv); material = sp.material_id;
        } else if (hit) {
            const rtx_plane & pl = s.planes[object - s.instance_count - s.sphere_count];
            rtxhp::plane_outputs(o, d, t, rtxnp::ptr3(pl.normal), rtxnp::ptr3(pl.u_axis), rtxnp::ptr3(pl.v_axis), point, normal, tu, tv); material = pl.material_id;
        }
        if (on(RTX_QUERY_DISTANCE) && out.distance) out.distance[e] = t;
        if (on(RTX_QUERY_POSITION) && out.position) { out.position[3 * e] = point.x; out.position[3 * e + 1] = point.y; out.position[3 * e + 2] = point.z; }
        if (on(RTX_QUERY_NORMAL) && out.normal) { out.normal[3 * e] = normal.x; out.normal[3 * e + 1] = normal.y; out.normal[3 * e + 2] = normal.z; }
        if (on(RTX_QUERY_UV) && out.uv) { out.uv[2 * e] = tu; out.uv[2 * e + 1] = tv; }
        if (on(RTX_QUERY_MATERIAL_ID) && out.material_id) out.material_id[e] = material;
        if (on(RTX_QUERY_OBJECT_ID) && out.object_id) out.object_id[e] = object;
        if (on(RTX_QUERY_TRIANGLE_ID) && out.triangle_id) out.triangle_id[e] = triangle;
    }
}
}  // namespace

static int query_hits_host(const rtxh_nearest_scene * scene, const float * segments, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                           int32_t * count_out, int32_t * stack_max_out, const HostMasks * km) {
    if (int rc = hits_args_check(scene, segments, n, max_hits, channels, out, count_out, true)) return rc;
    int high = 0;
    for (int64_t i = 0; i < n; i++) {
        HostNearestStack st;
        HostHitsList L;
        rtxhp::Tally w;
        if (km) { HostMasked<HostHitsScene> S(*scene, km->table, km->of_row(i)); rtxhp::walk(S, st, L, segments + 7 * i, max_hits, count_out != nullptr, w); }
        else { HostHitsScene S(*scene); rtxhp::walk(S, st, L, segments + 7 * i, max_hits, count_out != nullptr, w); }
        if (st.high > high) high = st.high;
        if (count_out) count_out[i] = w.count;
        if (max_hits) hit_write(*scene, segments + 7 * i, L, w.held, max_hits, i, channels, *out);
    }
    if (stack_max_out) *stack_max_out = high;
    return RTX_OK;
}

extern "C" int rtxh_query_hits(const rtxh_nearest_scene * scene, const float * segments, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                               int32_t * count_out, int32_t * stack_max_out) {
    return query_hits_host(scene, segments, n, max_hits, channels, out, count_out, stack_max_out, nullptr);
}
extern "C" int rtxh_query_hits_filtered(const rtxh_nearest_scene * scene, const float * segments, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                                        int32_t * count_out, int32_t * stack_max_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_hits_host(scene, segments, n, max_hits, channels, out, count_out, stack_max_out, &km);
}

static int query_hits_exhaustive_host(const rtxh_nearest_scene * scene, const float * segments, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                                      int32_t * count_out, const HostMasks km) {
    if (int rc = hits_args_check(scene, segments, n, max_hits, channels, out, count_out, false)) return rc;
    const rtxh_nearest_scene & s = *scene;
    for (int64_t i = 0; i < n; i++) {
        const float * row = segments + 7 * i;
        HostMasked<HostHitsScene> S(s, km.table, km.of_row(i));
        HostHitsList L;
        rtxhp::Tally w; w.count = 0; w.held = 0; w.bound = 0.0f;
        if (rtxhp::row_is_live(row) && S.row_visible()) {
            const rtxnp::P3 o = rtxnp::mk(row[0], row[1], row[2]), d = rtxnp::mk(row[3], row[4], row[5]);
            const float D = row[6];
            w.bound = D;
            rtxhp::world_primitives(S, L, max_hits, false, w, o, d, D);
            for (int k = 0; k < s.instance_count; k++) {
                if (!S.object_visible(k)) continue;
                const rtxnp::P3 co = rtxnp::xform_pos(s.instances[k].world_inv, o), cd = rtxnp::xform_dir(s.instances[k].world_inv, d);
                const rtxh_nearest_blas & B = s.blas[s.instances[k].blas_id];
                for (int t = 0; t < B.triangle_count; t++) {
                    float th, u, v;
                    if (rtxhp::tri_test(rtxnp::ptr3(B.hot[t].position_0), rtxnp::ptr3(B.hot[t].position_edge_1), rtxnp::ptr3(B.hot[t].position_edge_2), co, cd, D, th, u, v))
                        rtxhp::offer(L, max_hits, false, w, th, k, t);
                }
            }
        }
        if (count_out) count_out[i] = w.count;
        if (max_hits) hit_write(s, row, L, w.held, max_hits, i, channels, *out);
    }
    return RTX_OK;
}
extern "C" int rtxh_query_hits_exhaustive(const rtxh_nearest_scene * scene, const float * segments, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                                          int32_t * count_out) {
    return query_hits_exhaustive_host(scene, segments, n, max_hits, channels, out, count_out, kNoMasks);
}
extern "C" int rtxh_query_hits_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * segments, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                                                   int32_t * count_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_hits_exhaustive_host(scene, segments, n, max_hits, channels, out, count_out, km);
}

extern "C" float rtxh_hits_margin(float kappa, float scale) { return rtxhp::margin(kappa, scale); }

// =================================================================================================
// rtx_query_sweep on the host: rtxsp::walk (csrc/rtx_sweep_math.h) over the arrays of rtxh_query_nearest, and the exhaustive search
namespace {
// the channels of row i from its answer: what k_query_sweep stores — the nearest-point channels at the contact's centre, the distance t
void sweep_store(const rtxh_nearest_scene & s, const float * row, const rtxsp::Answer & a, int64_t i, uint32_t channels, const rtx_query_buffers & out) {
    const bool hit = a.kind != rtxnp::KIND_NONE;
    const rtxnp::P3 cc = rtxsp::centre_at(rtxnp::mk(row[0], row[1], row[2]), rtxnp::mk(row[3], row[4], row[5]), hit ? a.t : 0.0f);
    const float at[4] = { cc.x, cc.y, cc.z, 0.0f };
    rtxnp::Answer na; na.kind = a.kind; na.object = a.object; na.slot = a.slot; na.u = a.u; na.v = a.v; na.d2 = 0.0f;
    rtx_query_buffers o = out; o.distance = nullptr;
    nearest_store(s, at, na, i, channels, o);
    if ((channels & RTX_QUERY_DISTANCE) && out.distance) out.distance[i] = hit ? a.t : INFINITY;
}
}  // namespace

static int query_sweep_host(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, uint32_t channels, const rtx_query_buffers * out, int32_t * stack_max_out, const HostMasks * km) {
    if (int rc = nearest_scene_check(scene, sweeps, n, channels, out, true)) return rc;
    if (!scene_rigid(*scene)) return RTX_ERR_STATE;
    int high = 0;
    for (int64_t i = 0; i < n; i++) {
        HostNearestStack st;
        rtxsp::Answer a;
        if (km) { HostMasked<HostHitsScene> S(*scene, km->table, km->of_row(i)); rtxsp::walk(S, st, sweeps + 8 * i, a); }
        else { HostHitsScene S(*scene); rtxsp::walk(S, st, sweeps + 8 * i, a); }
        if (st.high > high) high = st.high;
        sweep_store(*scene, sweeps + 8 * i, a, i, channels, *out);
    }
    if (stack_max_out) *stack_max_out = high;
    return RTX_OK;
}

extern "C" int rtxh_query_sweep(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, uint32_t channels, const rtx_query_buffers * out, int32_t * stack_max_out) {
    return query_sweep_host(scene, sweeps, n, channels, out, stack_max_out, nullptr);
}
extern "C" int rtxh_query_sweep_filtered(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, uint32_t channels, const rtx_query_buffers * out, int32_t * stack_max_out,
                                         const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_sweep_host(scene, sweeps, n, channels, out, stack_max_out, &km);
}

static int query_sweep_exhaustive_host(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, uint32_t channels, const rtx_query_buffers * out, const HostMasks km) {
    if (int rc = nearest_scene_check(scene, sweeps, n, channels, out, false)) return rc;
    const rtxh_nearest_scene & s = *scene;
    for (int64_t i = 0; i < n; i++) {
        const float * row = sweeps + 8 * i;
        HostMasked<HostHitsScene> S(s, km.table, km.of_row(i));
        rtxsp::Answer a; rtxsp::clear(a);
        if (rtxsp::row_is_live(row) && S.row_visible()) {
            const rtxnp::P3 o = rtxnp::mk(row[0], row[1], row[2]), d = rtxnp::mk(row[3], row[4], row[5]);
            const float D = row[6], r = row[7];
            a.t = D;
            rtxsp::world_primitives(S, a, o, d, D, r);
            for (int k = 0; k < s.instance_count; k++) {
                if (!S.object_visible(k)) continue;
                const rtxnp::P3 co = rtxnp::xform_pos(s.instances[k].world_inv, o), cd = rtxnp::xform_dir(s.instances[k].world_inv, d);
                const rtxh_nearest_blas & B = s.blas[s.instances[k].blas_id];
                for (int j = 0; j < B.triangle_count; j++) {
                    float t, u, v, d20;
                    if (rtxsp::triangle_sweep(rtxnp::ptr3(B.hot[j].position_0), rtxnp::ptr3(B.hot[j].position_edge_1), rtxnp::ptr3(B.hot[j].position_edge_2), co, cd, r, a.t, t, u, v, d20))
                        rtxsp::offer(a, D, t, d20, rtxnp::KIND_TRI, k, j, u, v);
                }
            }
        }
        sweep_store(s, row, a, i, channels, *out);
    }
    return RTX_OK;
}
extern "C" int rtxh_query_sweep_exhaustive(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, uint32_t channels, const rtx_query_buffers * out) {
    return query_sweep_exhaustive_host(scene, sweeps, n, channels, out, kNoMasks);
}
extern "C" int rtxh_query_sweep_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                                    const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_sweep_exhaustive_host(scene, sweeps, n, channels, out, km);
}

extern "C" float rtxh_sweep_bound(float local_scale, float world_scale, float travelled, float radius) { return rtxsp::sweep_bound(local_scale, world_scale, travelled, radius); }
extern "C" int rtxh_sweep_triangle(const float origin[3], const float direction[3], float radius, float bound, const rtx_triangle_hot * tri, float * t_out, float uv_out[2], float * d20_out) {
    float t = 0.0f, u = 0.0f, v = 0.0f, d20 = 0.0f;
    const bool any = rtxsp::triangle_sweep(rtxnp::ptr3(tri->position_0), rtxnp::ptr3(tri->position_edge_1), rtxnp::ptr3(tri->position_edge_2), rtxnp::ptr3(origin), rtxnp::ptr3(direction), radius, bound, t, u, v, d20);
    if (any) { *t_out = t; uv_out[0] = u; uv_out[1] = v; *d20_out = d20; }
    return any ? 1 : 0;
}
extern "C" int rtxh_sweep_sphere(const float origin[3], const float direction[3], float radius, const rtx_sphere * sphere, float * t_out, float * d20_out) {
    float t = 0.0f, d20 = 0.0f;
    const bool any = rtxsp::sphere_sweep(rtxnp::ptr3(sphere->center), sphere->radius_squared, rtxnp::ptr3(origin), rtxnp::ptr3(direction), radius, t, d20);
    if (any) { *t_out = t; *d20_out = d20; }
    return any ? 1 : 0;
}
extern "C" int rtxh_sweep_plane(const float origin[3], const float direction[3], float radius, const rtx_plane * plane, float * t_out, float * d20_out) {
    float t = 0.0f, d20 = 0.0f;
    const bool any = rtxsp::plane_sweep(rtxnp::ptr3(plane->normal), plane->distance, rtxnp::ptr3(origin), rtxnp::ptr3(direction), radius, t, d20);
    if (any) { *t_out = t; *d20_out = d20; }
    return any ? 1 : 0;
}

// =================================================================================================
// rtx_query_overlap on the host: rtxop::walk (csrc/rtx_overlap_math.h) over the arrays of rtxh_query_nearest, and the exhaustive search
namespace {
struct HostOverlapScene : HostNearestScene {
    explicit HostOverlapScene(const rtxh_nearest_scene & sc) : HostNearestScene{ sc } {}
    int instance_count() const { return s.instance_count; }
    int enter(int slot, rtxop::Frame & F) {
        const int inst = s.tlas_indices[slot];
        F = rtxop::local_frame(F, s.instances[inst].world_inv);
        B = &s.blas[s.instances[inst].blas_id];
        return inst;
    }
};
struct HostOverlapStack {
    int node[RTX_MAX_STACK]; int high = 0;
    void push(int sp, int n) { node[sp] = n; if (sp + 1 > high) high = sp + 1; }
    void pop(int sp, int & n) const { n = node[sp]; }
};
struct HostOverlapList {
    int32_t object[rtxop::MAX_HITS], triangle[rtxop::MAX_HITS];
    void get(int j, int32_t & o_, int32_t & s_) const { o_ = object[j]; s_ = triangle[j]; }
    void set(int j, int32_t o_, int32_t s_) { object[j] = o_; triangle[j] = s_; }
};
// the argument rules of rtx_query_overlap, in its order
int overlap_args_check(const rtxh_nearest_scene * s, const float * boxes, int64_t n, int32_t max_hits, const int32_t * object_out, const int32_t * triangle_out, const int32_t * count_out,
                       uint32_t flags, bool trees) {
    const bool any = (flags & RTX_OVERLAP_ANY) != 0, objects = (flags & RTX_OVERLAP_OBJECTS) != 0;
    if (max_hits < 0 || max_hits > rtxop::MAX_HITS) return RTX_ERR_INVALID_ARG;
    if (any && (max_hits != 0 || objects)) return RTX_ERR_INVALID_ARG;
    if (objects && triangle_out) return RTX_ERR_INVALID_ARG;
    if (max_hits == 0 && !count_out) return RTX_ERR_INVALID_ARG;
    if (max_hits > 0 && !object_out && !triangle_out) return RTX_ERR_INVALID_ARG;
    if (flags & ~((uint32_t)RTX_QUERY_SORT | (uint32_t)RTX_OVERLAP_OBJECTS | (uint32_t)RTX_OVERLAP_ANY)) return RTX_ERR_INVALID_ARG;
    const rtx_query_buffers none = {};
    return nearest_scene_check(s, boxes, n, (uint32_t)RTX_QUERY_DISTANCE, &none, trees);
}
// the K entries of row i from its list, and its count: what k_query_overlap stores
void overlap_write(const HostOverlapList & L, const rtxop::Tally & w, int K, int64_t i, int32_t * object_out, int32_t * triangle_out, int32_t * count_out) {
    if (count_out) count_out[i] = w.count;
    for (int j = 0; j < K; j++) {
        const size_t e = (size_t)i * (size_t)K + (size_t)j;
        if (object_out) object_out[e] = j < w.held ? L.object[j] : -1;
        if (triangle_out) triangle_out[e] = j < w.held ? L.triangle[j] : -1;
    }
}
template <int FORM, typename Scene>
void overlap_exhaustive_row(const rtxh_nearest_scene & s, Scene & S, HostOverlapList & L, const float * row, int K, rtxop::Tally & w) {
    w.count = 0; w.held = 0;
    if (!rtxop::row_is_live(row) || !S.row_visible()) return;
    const rtxop::Frame W = rtxop::world_frame(row);
    if (rtxop::world_primitives<FORM>(S, L, K, w, W)) return;
    for (int k = 0; k < s.instance_count; k++) {
        if (!S.object_visible(k)) continue;
        const rtxop::Frame F = rtxop::local_frame(W, s.instances[k].world_inv);
        const rtxh_nearest_blas & B = s.blas[s.instances[k].blas_id];
        for (int t = 0; t < B.triangle_count; t++) {
            if (!rtxop::triangle_overlaps(F, rtxnp::ptr3(B.hot[t].position_0), rtxnp::ptr3(B.hot[t].position_edge_1), rtxnp::ptr3(B.hot[t].position_edge_2))) continue;
            if (FORM == rtxop::FORM_TRIANGLES) { rtxop::offer(L, K, w, k, t); continue; }
            rtxop::offer(L, K, w, k, -1);
            if (FORM == rtxop::FORM_ANY) return;
            break;
        }
    }
}
}  // namespace

static int query_overlap_host(const rtxh_nearest_scene * scene, const float * boxes, int64_t n, int32_t max_hits, int32_t * object_out, int32_t * triangle_out, int32_t * count_out,
                              uint32_t flags, int32_t * stack_max_out, const HostMasks * km) {
    if (int rc = overlap_args_check(scene, boxes, n, max_hits, object_out, triangle_out, count_out, flags, true)) return rc;
    if (!scene_rigid(*scene)) return RTX_ERR_STATE;
    const int form = (flags & RTX_OVERLAP_ANY) ? rtxop::FORM_ANY : (flags & RTX_OVERLAP_OBJECTS) ? rtxop::FORM_OBJECTS : rtxop::FORM_TRIANGLES;
    int high = 0;
    for (int64_t i = 0; i < n; i++) {
        HostOverlapStack st;
        HostOverlapList L;
        rtxop::Tally w;
        const float * row = boxes + rtxop::ROW_FLOATS * i;
        auto run = [&](auto & S) {
            if (form == rtxop::FORM_ANY) rtxop::walk<rtxop::FORM_ANY>(S, st, L, row, 0, w);
            else if (form == rtxop::FORM_OBJECTS) rtxop::walk<rtxop::FORM_OBJECTS>(S, st, L, row, max_hits, w);
            else rtxop::walk<rtxop::FORM_TRIANGLES>(S, st, L, row, max_hits, w);
        };
        if (km) { HostMasked<HostOverlapScene> S(*scene, km->table, km->of_row(i)); run(S); }
        else { HostOverlapScene S(*scene); run(S); }
        if (st.high > high) high = st.high;
        overlap_write(L, w, max_hits, i, object_out, triangle_out, count_out);
    }
    if (stack_max_out) *stack_max_out = high;
    return RTX_OK;
}
extern "C" int rtxh_query_overlap(const rtxh_nearest_scene * scene, const float * boxes, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                  int32_t * count_out, uint32_t flags, int32_t * stack_max_out) {
    return query_overlap_host(scene, boxes, n, max_hits, object_id_out, triangle_id_out, count_out, flags, stack_max_out, nullptr);
}
extern "C" int rtxh_query_overlap_filtered(const rtxh_nearest_scene * scene, const float * boxes, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                           int32_t * count_out, uint32_t flags, int32_t * stack_max_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_overlap_host(scene, boxes, n, max_hits, object_id_out, triangle_id_out, count_out, flags, stack_max_out, &km);
}

static int query_overlap_exhaustive_host(const rtxh_nearest_scene * scene, const float * boxes, int64_t n, int32_t max_hits, int32_t * object_out, int32_t * triangle_out,
                                         int32_t * count_out, uint32_t flags, const HostMasks km) {
    if (int rc = overlap_args_check(scene, boxes, n, max_hits, object_out, triangle_out, count_out, flags, false)) return rc;
    const rtxh_nearest_scene & s = *scene;
    for (int64_t i = 0; i < n; i++) {
        const float * row = boxes + rtxop::ROW_FLOATS * i;
        HostMasked<HostOverlapScene> S(s, km.table, km.of_row(i));
        HostOverlapList L;
        rtxop::Tally w;
        if (flags & RTX_OVERLAP_ANY) overlap_exhaustive_row<rtxop::FORM_ANY>(s, S, L, row, 0, w);
        else if (flags & RTX_OVERLAP_OBJECTS) overlap_exhaustive_row<rtxop::FORM_OBJECTS>(s, S, L, row, max_hits, w);
        else overlap_exhaustive_row<rtxop::FORM_TRIANGLES>(s, S, L, row, max_hits, w);
        overlap_write(L, w, max_hits, i, object_out, triangle_out, count_out);
    }
    return RTX_OK;
}
extern "C" int rtxh_query_overlap_exhaustive(const rtxh_nearest_scene * scene, const float * boxes, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                             int32_t * count_out, uint32_t flags) {
    return query_overlap_exhaustive_host(scene, boxes, n, max_hits, object_id_out, triangle_id_out, count_out, flags, kNoMasks);
}
extern "C" int rtxh_query_overlap_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * boxes, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                                      int32_t * count_out, uint32_t flags, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_overlap_exhaustive_host(scene, boxes, n, max_hits, object_id_out, triangle_id_out, count_out, flags, km);
}
extern "C" float rtxh_overlap_margin(float local_scale, float world_scale, float kappa) { return rtxop::margin(local_scale, world_scale, kappa); }

// =================================================================================================
// rtx_query_overlap_capsule on the host: rtxcp::walk (csrc/rtx_capsule_math.h) over the arrays of rtxh_query_nearest, and the exhaustive
// search; the stack, the list, the argument rules and the stores are rtx_query_overlap's above
namespace {
struct HostCapsuleScene : HostNearestScene {
    explicit HostCapsuleScene(const rtxh_nearest_scene & sc) : HostNearestScene{ sc } {}
    int instance_count() const { return s.instance_count; }
    int enter(int slot, rtxcp::Frame & F) {
        const int inst = s.tlas_indices[slot];
        F = rtxcp::local_frame(F, s.instances[inst].world_inv);
        B = &s.blas[s.instances[inst].blas_id];
        return inst;
    }
};
template <int FORM, typename Scene>
void capsule_exhaustive_row(const rtxh_nearest_scene & s, Scene & S, HostOverlapList & L, const float * row, int K, rtxop::Tally & w) {
    w.count = 0; w.held = 0;
    if (!rtxcp::row_is_live(row) || !S.row_visible()) return;
    const rtxcp::Frame W = rtxcp::world_frame(row);
    if (rtxcp::world_primitives<FORM>(S, L, K, w, W)) return;
    for (int k = 0; k < s.instance_count; k++) {
        if (!S.object_visible(k)) continue;
        const rtxcp::Frame F = rtxcp::local_frame(W, s.instances[k].world_inv);
        const rtxh_nearest_blas & B = s.blas[s.instances[k].blas_id];
        for (int t = 0; t < B.triangle_count; t++) {
            if (!rtxcp::triangle_overlaps(F, rtxnp::ptr3(B.hot[t].position_0), rtxnp::ptr3(B.hot[t].position_edge_1), rtxnp::ptr3(B.hot[t].position_edge_2))) continue;
            if (FORM == rtxcp::FORM_TRIANGLES) { rtxop::offer(L, K, w, k, t); continue; }
            rtxop::offer(L, K, w, k, -1);
            if (FORM == rtxcp::FORM_ANY) return;
            break;
        }
    }
}
}  // namespace

static int query_overlap_capsule_host(const rtxh_nearest_scene * scene, const float * capsules, int64_t n, int32_t max_hits, int32_t * object_out, int32_t * triangle_out, int32_t * count_out,
                                      uint32_t flags, int32_t * stack_max_out, const HostMasks * km) {
    if (int rc = overlap_args_check(scene, capsules, n, max_hits, object_out, triangle_out, count_out, flags, true)) return rc;
    if (!scene_rigid(*scene)) return RTX_ERR_STATE;
    const int form = (flags & RTX_OVERLAP_ANY) ? rtxcp::FORM_ANY : (flags & RTX_OVERLAP_OBJECTS) ? rtxcp::FORM_OBJECTS : rtxcp::FORM_TRIANGLES;
    int high = 0;
    for (int64_t i = 0; i < n; i++) {
        HostOverlapStack st;
        HostOverlapList L;
        rtxop::Tally w;
        const float * row = capsules + rtxcp::ROW_FLOATS * i;
        auto run = [&](auto & S) {
            if (form == rtxcp::FORM_ANY) rtxcp::walk<rtxcp::FORM_ANY>(S, st, L, row, 0, w);
            else if (form == rtxcp::FORM_OBJECTS) rtxcp::walk<rtxcp::FORM_OBJECTS>(S, st, L, row, max_hits, w);
            else rtxcp::walk<rtxcp::FORM_TRIANGLES>(S, st, L, row, max_hits, w);
        };
        if (km) { HostMasked<HostCapsuleScene> S(*scene, km->table, km->of_row(i)); run(S); }
        else { HostCapsuleScene S(*scene); run(S); }
        if (st.high > high) high = st.high;
        overlap_write(L, w, max_hits, i, object_out, triangle_out, count_out);
    }
    if (stack_max_out) *stack_max_out = high;
    return RTX_OK;
}
extern "C" int rtxh_query_overlap_capsule(const rtxh_nearest_scene * scene, const float * capsules, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                          int32_t * count_out, uint32_t flags, int32_t * stack_max_out) {
    return query_overlap_capsule_host(scene, capsules, n, max_hits, object_id_out, triangle_id_out, count_out, flags, stack_max_out, nullptr);
}
extern "C" int rtxh_query_overlap_capsule_filtered(const rtxh_nearest_scene * scene, const float * capsules, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                                   int32_t * count_out, uint32_t flags, int32_t * stack_max_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_overlap_capsule_host(scene, capsules, n, max_hits, object_id_out, triangle_id_out, count_out, flags, stack_max_out, &km);
}

static int query_overlap_capsule_exhaustive_host(const rtxh_nearest_scene * scene, const float * capsules, int64_t n, int32_t max_hits, int32_t * object_out, int32_t * triangle_out,
                                                 int32_t * count_out, uint32_t flags, const HostMasks km) {
    if (int rc = overlap_args_check(scene, capsules, n, max_hits, object_out, triangle_out, count_out, flags, false)) return rc;
    const rtxh_nearest_scene & s = *scene;
    for (int64_t i = 0; i < n; i++) {
        const float * row = capsules + rtxcp::ROW_FLOATS * i;
        HostMasked<HostCapsuleScene> S(s, km.table, km.of_row(i));
        HostOverlapList L;
        rtxop::Tally w;
        if (flags & RTX_OVERLAP_ANY) capsule_exhaustive_row<rtxcp::FORM_ANY>(s, S, L, row, 0, w);
        else if (flags & RTX_OVERLAP_OBJECTS) capsule_exhaustive_row<rtxcp::FORM_OBJECTS>(s, S, L, row, max_hits, w);
        else capsule_exhaustive_row<rtxcp::FORM_TRIANGLES>(s, S, L, row, max_hits, w);
        overlap_write(L, w, max_hits, i, object_out, triangle_out, count_out);
    }
    return RTX_OK;
}
extern "C" int rtxh_query_overlap_capsule_exhaustive(const rtxh_nearest_scene * scene, const float * capsules, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                                     int32_t * count_out, uint32_t flags) {
    return query_overlap_capsule_exhaustive_host(scene, capsules, n, max_hits, object_id_out, triangle_id_out, count_out, flags, kNoMasks);
}
extern "C" int rtxh_query_overlap_capsule_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * capsules, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                                              int32_t * count_out, uint32_t flags, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    return query_overlap_capsule_exhaustive_host(scene, capsules, n, max_hits, object_id_out, triangle_id_out, count_out, flags, km);
}
extern "C" float rtxh_capsule_margin(float local_scale, float world_scale, float kappa) { return rtxcp::margin(local_scale, world_scale, kappa); }

// =================================================================================================
// rtx_query_sweep_box on the host: rtxbs::walk (csrc/rtx_boxsweep_math.h) over the arrays of rtxh_query_nearest, and the exhaustive search
namespace {
struct HostBoxSweepScene : HostNearestScene {
    explicit HostBoxSweepScene(const rtxh_nearest_scene & sc) : HostNearestScene{ sc } {}
    int instance_count() const { return s.instance_count; }
    int enter(int slot, rtxop::Frame & F, rtxnp::P3 & cd) {
        const int inst = s.tlas_indices[slot];
        F = rtxop::local_frame(F, s.instances[inst].world_inv);
        cd = rtxnp::xform_dir(s.instances[inst].world_inv, cd);
        B = &s.blas[s.instances[inst].blas_id];
        return inst;
    }
};
struct HostBoxSweepOut { float * t; float * normal; int32_t * object_id; int32_t * triangle_id; int32_t * axis; };
int sweep_box_args_check(const rtxh_nearest_scene * s, const float * sweeps, int64_t n, const HostBoxSweepOut & o, bool trees) {
    if (!o.t && !o.normal && !o.object_id && !o.triangle_id && !o.axis) return RTX_ERR_INVALID_ARG;
    const rtx_query_buffers none = {};
    return nearest_scene_check(s, sweeps, n, (uint32_t)RTX_QUERY_DISTANCE, &none, trees);
}
// the outputs of row i from its answer: what k_query_sweep_box stores
void sweep_box_store(const rtxh_nearest_scene & s, const float * row, const rtxbs::Answer & a, int64_t i, const HostBoxSweepOut & o) {
    if (o.t) o.t[i] = a.t;
    if (o.normal) {
        rtxnp::P3 n = rtxnp::mk(0.0f, 0.0f, 0.0f);
        if (a.object >= 0 && a.t != 0.0f) {
            const rtxop::Frame W = rtxbs::world_frame(row);
            const rtxnp::P3 d = rtxnp::mk(row[3], row[4], row[5]);
            if (a.slot >= 0) {
                const rtx_instance & I = s.instances[a.object];
                const rtx_triangle_hot & h = s.blas[I.blas_id].hot[a.slot];
                n = rtxbs::triangle_normal(W, I.world_inv, rtxnp::ptr3(h.position_edge_1), rtxnp::ptr3(h.position_edge_2), a.axis, d);
            } else if (a.axis == rtxbs::AXIS_SPHERE) {
                const rtx_sphere & sp = s.spheres[a.object - s.instance_count];
                n = rtxbs::sphere_normal(W, d, rtxnp::ptr3(sp.center), sp.radius_squared, a.t);
            } else {
                const rtx_plane & pl = s.planes[a.object - s.instance_count - s.sphere_count];
                n = rtxbs::plane_normal(W, rtxnp::ptr3(pl.normal), pl.distance);
            }
        }
        o.normal[3 * i] = n.x; o.normal[3 * i + 1] = n.y; o.normal[3 * i + 2] = n.z;
    }
    if (o.object_id) o.object_id[i] = a.object;
    if (o.triangle_id) o.triangle_id[i] = a.slot;
    if (o.axis) o.axis[i] = a.axis;
}
}  // namespace

static int query_sweep_box_host(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, const HostBoxSweepOut & o, int32_t * stack_max_out, const HostMasks * km) {
    if (int rc = sweep_box_args_check(scene, sweeps, n, o, true)) return rc;
    if (!scene_rigid(*scene)) return RTX_ERR_STATE;
    int high = 0;
    for (int64_t i = 0; i < n; i++) {
        HostNearestStack st;
        rtxbs::Answer a;
        const float * row = sweeps + rtxbs::ROW_FLOATS * i;
        if (km) { HostMasked<HostBoxSweepScene> S(*scene, km->table, km->of_row(i)); rtxbs::walk(S, st, row, a); }
        else { HostBoxSweepScene S(*scene); rtxbs::walk(S, st, row, a); }
        if (st.high > high) high = st.high;
        sweep_box_store(*scene, row, a, i, o);
    }
    if (stack_max_out) *stack_max_out = high;
    return RTX_OK;
}
extern "C" int rtxh_query_sweep_box(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, float * t_out, float * normal_out, int32_t * object_id_out, int32_t * triangle_id_out,
                                    int32_t * axis_out, int32_t * stack_max_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    const HostBoxSweepOut o = { t_out, normal_out, object_id_out, triangle_id_out, axis_out };
    return query_sweep_box_host(scene, sweeps, n, o, stack_max_out, &km);
}
extern "C" int rtxh_query_sweep_box_exhaustive(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, float * t_out, float * normal_out, int32_t * object_id_out,
                                               int32_t * triangle_id_out, int32_t * axis_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask) {
    const HostMasks km = { object_masks, row_masks, row_mask };
    const HostBoxSweepOut o = { t_out, normal_out, object_id_out, triangle_id_out, axis_out };
    if (int rc = sweep_box_args_check(scene, sweeps, n, o, false)) return rc;
    const rtxh_nearest_scene & s = *scene;
    for (int64_t i = 0; i < n; i++) {
        const float * row = sweeps + rtxbs::ROW_FLOATS * i;
        HostMasked<HostBoxSweepScene> S(s, km.table, km.of_row(i));
        rtxbs::Answer a; rtxbs::clear(a);
        if (rtxbs::row_is_live(row) && S.row_visible()) {
            const float D = row[6];
            a.t = D;
            const rtxop::Frame W = rtxbs::world_frame(row);
            const rtxnp::P3 d = rtxnp::mk(row[3], row[4], row[5]);
            rtxbs::world_primitives(S, a, W, d, rtxop::to_box(W, d), D);
            for (int k = 0; k < s.instance_count; k++) {
                if (!S.object_visible(k)) continue;
                const rtxop::Frame F = rtxop::local_frame(W, s.instances[k].world_inv);
                const rtxnp::P3 w = rtxop::to_box(F, rtxnp::xform_dir(s.instances[k].world_inv, d));
                const rtxh_nearest_blas & B = s.blas[s.instances[k].blas_id];
                for (int j = 0; j < B.triangle_count; j++) {
                    float t; int axis;
                    if (rtxbs::triangle_sweep(F, w, rtxnp::ptr3(B.hot[j].position_0), rtxnp::ptr3(B.hot[j].position_edge_1), rtxnp::ptr3(B.hot[j].position_edge_2), a.t, t, axis))
                        rtxbs::offer(a, D, t, k, j, axis);
                }
            }
            rtxbs::finish(a);
        }
        sweep_box_store(s, row, a, i, o);
    }
    return RTX_OK;
}
extern "C" float rtxh_sweep_box_bound(float local_scale, float world_scale, float travelled, float kappa) { return rtxbs::sweep_box_bound(local_scale, world_scale, travelled, kappa); }
// the candidate functions at a row's WORLD frame (an identity instance): 1 and (t, axis) when the primitive yields a candidate, else 0
extern "C" int rtxh_sweep_box_triangle(const float row[14], float bound, const rtx_triangle_hot * tri, float * t_out, int32_t * axis_out) {
    const rtxop::Frame W = rtxbs::world_frame(row);
    float t = 0.0f; int axis = -1;
    const bool any = rtxbs::triangle_sweep(W, rtxop::to_box(W, rtxnp::ptr3(row + 3)), rtxnp::ptr3(tri->position_0), rtxnp::ptr3(tri->position_edge_1), rtxnp::ptr3(tri->position_edge_2), bound, t, axis);
    if (any) { *t_out = t; *axis_out = axis; }
    return any ? 1 : 0;
}
extern "C" int rtxh_sweep_box_sphere(const float row[14], float bound, const rtx_sphere * sphere, float * t_out) {
    const rtxop::Frame W = rtxbs::world_frame(row);
    float t = 0.0f;
    const bool any = rtxbs::sphere_sweep(W, rtxop::to_box(W, rtxnp::ptr3(row + 3)), rtxnp::ptr3(sphere->center), sphere->radius_squared, bound, t);
    if (any) *t_out = t;
    return any ? 1 : 0;
}
extern "C" int rtxh_sweep_box_plane(const float row[14], const rtx_plane * plane, float * t_out) {
    const rtxop::Frame W = rtxbs::world_frame(row);
    float t = 0.0f;
    const bool any = rtxbs::plane_sweep(W, rtxnp::ptr3(row + 3), rtxnp::ptr3(plane->normal), plane->distance, t);
    if (any) *t_out = t;
    return any ? 1 : 0;
}

// =================================================================================================
// Procedural atrium: a seeded Sponza-class stand-in (the real sponza.obj is absent from the mount).
// Colonnaded hall with arches, balustrades, curtains, vases and rough "statues"; triangle sizes span
// three orders of magnitude on purpose (large wall quads next to finely tessellated ornaments).
namespace {
struct MeshOut {
    std::vector<float> pos, nrm, uv; std::vector<int> mat;
    void tri(V a, V b, V c, V na, V nb, V nc, float ua, float va, float ub, float vb, float uc, float vc, int m) {
        const V p[3] = { a, b, c }, n[3] = { na, nb, nc };
        for (int k = 0; k < 3; k++) { pos.push_back(p[k].x); pos.push_back(p[k].y); pos.push_back(p[k].z); nrm.push_back(n[k].x); nrm.push_back(n[k].y); nrm.push_back(n[k].z); }
        // texture v is stored flipped, as the reference's loader does (OBJLoader.cpp:139-141)
        uv.push_back(ua); uv.push_back(1.0f - va); uv.push_back(ub); uv.push_back(1.0f - vb); uv.push_back(uc); uv.push_back(1.0f - vc);
        mat.push_back(m);
    }
};
inline V norm(V v) { float l = sqrtf(dot(v, v)); return l > 0 ? v * (1.0f / l) : mk(0, 1, 0); }

struct Rng { uint32_t s; float next() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f); } };

// parametric surface patch: P(u,v), N(u,v) sampled on an (nu x nv) grid
template <typename F>
void patch(MeshOut & m, int nu, int nv, int material, float uscale, float vscale, bool flip, F && f) {
    std::vector<V> P((size_t)(nu + 1) * (nv + 1)), N(P.size());
    for (int j = 0; j <= nv; j++) for (int i = 0; i <= nu; i++) f((float)i / nu, (float)j / nv, P[(size_t)j * (nu + 1) + i], N[(size_t)j * (nu + 1) + i]);
    for (int j = 0; j < nv; j++) for (int i = 0; i < nu; i++) {
        const size_t a = (size_t)j * (nu + 1) + i, b = a + 1, c = a + (nu + 1), d = c + 1;
        const float u0 = uscale * i / nu, u1 = uscale * (i + 1) / nu, v0 = vscale * j / nv, v1 = vscale * (j + 1) / nv;
        if (!flip) { m.tri(P[a], P[b], P[d], N[a], N[b], N[d], u0, v0, u1, v0, u1, v1, material); m.tri(P[a], P[d], P[c], N[a], N[d], N[c], u0, v0, u1, v1, u0, v1, material); }
        else       { m.tri(P[a], P[d], P[b], N[a], N[d], N[b], u0, v0, u1, v1, u1, v0, material); m.tri(P[a], P[c], P[d], N[a], N[c], N[d], u0, v0, u0, v1, u1, v1, material); }
    }
}
inline float hash2(int x, int y, uint32_t seed) { uint32_t h = (uint32_t)x * 374761393u + (uint32_t)y * 668265263u + seed * 2246822519u; h = (h ^ (h >> 13)) * 1274126177u; h ^= h >> 16; return (float)(h & 0xffffff) * (1.0f / 16777216.0f); }
inline float vnoise(float x, float y, uint32_t seed) {
    const int xi = (int)floorf(x), yi = (int)floorf(y); const float fx = x - xi, fy = y - yi;
    const float sx = fx * fx * (3 - 2 * fx), sy = fy * fy * (3 - 2 * fy);
    const float a = hash2(xi, yi, seed), b = hash2(xi + 1, yi, seed), c = hash2(xi, yi + 1, seed), d = hash2(xi + 1, yi + 1, seed);
    return (a + (b - a) * sx) + ((c + (d - c) * sx) - (a + (b - a) * sx)) * sy;
}
}  // namespace

extern "C" int rtxh_atrium_generate(uint32_t seed, int32_t detail, rtxh_mesh * out) {
    if (!out || detail < 0 || detail > 8) return RTX_ERR_INVALID_ARG;
    MeshOut m; Rng rng = { seed };
    const float PI = 3.14159265358979f;
    // tessellation multiplier: detail 1 ~ 255k triangles (the cfg3 size), detail 0 ~ 64k, detail 4 ~ 1.6M
    const float q = 0.25f * (float)(detail + 1);
    auto T = [&](int base) { int v = (int)(base * q + 0.5f); return v < 2 ? 2 : v; };
    const float HX = 30.0f, HZ = 12.0f, HY = 18.0f;
    enum { M_FLOOR, M_WALL, M_ENDWALL, M_COLUMN, M_CAPITAL, M_ARCH, M_BALUSTER, M_CURTAIN0, M_VASE0 = M_CURTAIN0 + 6, M_STATUE0 = M_VASE0 + 4, M_TRIM = M_STATUE0 + 4, M_COUNT = M_TRIM + 4 };

    // floor: gently uneven flagstones, normals from the height field
    patch(m, T(320), T(128), M_FLOOR, 30.0f, 12.0f, false, [&](float u, float v, V & P, V & N) {
        const float x = -HX + 2 * HX * u, z = -HZ + 2 * HZ * v;
        auto h = [&](float xx, float zz) { return 0.03f * vnoise(xx * 1.7f, zz * 1.7f, seed) + 0.01f * vnoise(xx * 9.1f, zz * 7.7f, seed + 1); };
        P = mk(x, h(x, z), z);
        const float e = 0.05f; N = norm(mk(h(x - e, z) - h(x + e, z), 2 * e, h(x, z - e) - h(x, z + e)));
    });
    // side walls with relief, facing inward
    for (int side = 0; side < 2; side++) {
        const float zs = side ? HZ : -HZ, sgn = side ? -1.0f : 1.0f;
        patch(m, T(240), T(80), M_WALL, 24.0f, 8.0f, side == 0, [&](float u, float v, V & P, V & N) {
            const float x = -HX + 2 * HX * u, y = HY * v;
            auto r = [&](float xx, float yy) { return 0.12f * vnoise(xx * 0.9f, yy * 0.9f, seed + 7 + side) + 0.02f * vnoise(xx * 6.3f, yy * 6.1f, seed + 9); };
            P = mk(x, y, zs + sgn * r(x, y));
            const float e = 0.05f; N = norm(mk(sgn * (r(x - e, y) - r(x + e, y)), sgn * (r(x, y - e) - r(x, y + e)), sgn * 2 * e));
        });
    }
    // end walls (large flat quads: big triangles)
    for (int side = 0; side < 2; side++) {
        const float xs = side ? HX : -HX, sgn = side ? -1.0f : 1.0f;
        patch(m, T(24), T(20), M_ENDWALL, 10.0f, 8.0f, side == 1, [&](float u, float v, V & P, V & N) {
            P = mk(xs, HY * v, -HZ + 2 * HZ * u); N = mk(sgn, 0, 0);
        });
    }
    // two rows of columns with capitals, arches between neighbours
    const int NCOL = 10;
    for (int row = 0; row < 2; row++) {
        const float cz = row ? 7.0f : -7.0f;
        for (int c = 0; c < NCOL; c++) {
            const float cx = -HX + 3.0f + c * ((2 * HX - 6.0f) / (NCOL - 1));
            const float rad = 0.8f, hgt = 10.0f;
            patch(m, T(96), T(80), M_COLUMN, 4.0f, 10.0f, true, [&](float u, float v, V & P, V & N) {
                const float a = 2 * PI * u, fl = 1.0f + 0.04f * cosf(16.0f * a);      // fluted shaft
                const float r = rad * fl * (1.0f - 0.12f * v);
                P = mk(cx + r * cosf(a), hgt * v, cz + r * sinf(a)); N = norm(mk(cosf(a), 0.1f, sinf(a)));
            });
            patch(m, T(96), T(32), M_CAPITAL, 4.0f, 1.0f, true, [&](float u, float v, V & P, V & N) {
                const float a = 2 * PI * u, b = PI * (v - 0.5f);
                const float R = 0.95f + 0.35f * cosf(b);
                P = mk(cx + R * cosf(a), hgt + 0.35f + 0.35f * sinf(b), cz + R * sinf(a)); N = norm(mk(cosf(a) * cosf(b), sinf(b), sinf(a) * cosf(b)));
            });
            if (c + 1 < NCOL) {
                const float span = (2 * HX - 6.0f) / (NCOL - 1), mx = cx + 0.5f * span;
                patch(m, T(64), T(32), M_ARCH, 6.0f, 2.0f, true, [&](float u, float v, V & P, V & N) {
                    const float a = PI * u, b = 2 * PI * v, R = 0.5f * span, r = 0.45f;
                    const V cdir = mk(-cosf(a), sinf(a), 0.0f);
                    P = mk(mx, hgt + 0.7f, cz) + cdir * (R + r * cosf(b)) + mk(0, 0, r * sinf(b));
                    N = norm(cdir * cosf(b) + mk(0, 0, sinf(b)));
                });
            }
        }
    }
    // gallery balustrades: many small balusters
    for (int row = 0; row < 2; row++) {
        const float bz = row ? 8.2f : -8.2f;
        const int NB = 60;
        for (int b = 0; b < NB; b++) {
            const float bx = -HX + 1.5f + b * ((2 * HX - 3.0f) / (NB - 1));
            patch(m, T(24), T(20), M_BALUSTER, 1.0f, 1.0f, true, [&](float u, float v, V & P, V & N) {
                const float a = 2 * PI * u, r = 0.09f + 0.06f * sinf(PI * v) * sinf(PI * v) + 0.03f * cosf(6 * PI * v);
                P = mk(bx + r * cosf(a), 12.0f + 1.1f * v, bz + r * sinf(a)); N = norm(mk(cosf(a), 0.2f * cosf(PI * v), sinf(a)));
            });
        }
        patch(m, T(120), 2, M_TRIM, 30.0f, 0.2f, false, [&](float u, float v, V & P, V & N) {   // hand rail
            P = mk(-HX + 1.5f + (2 * HX - 3.0f) * u, 13.15f, bz - 0.12f + 0.24f * v); N = mk(0, 1, 0);
        });
    }
    // curtains: wavy sheets hanging between columns
    for (int k = 0; k < 6; k++) {
        const float cx0 = -24.0f + k * 9.0f, cz = (k & 1) ? 7.6f : -7.6f;
        const float ph = rng.next() * 6.28f;
        patch(m, T(80), T(120), M_CURTAIN0 + k, 3.0f, 5.0f, (k & 1) != 0, [&](float u, float v, V & P, V & N) {
            const float x = cx0 + 5.0f * u, y = 11.5f - 8.5f * v;
            auto w = [&](float uu, float vv) { return 0.28f * sinf(14.0f * uu + ph) * (0.3f + 0.7f * vv) + 0.05f * sinf(40.0f * uu + 3.0f * vv); };
            P = mk(x, y, cz + w(u, v));
            const float e = 0.002f; const float dzdu = (w(u + e, v) - w(u - e, v)) / (2 * e * 5.0f), dzdv = (w(u, v + e) - w(u, v - e)) / (2 * e * -8.5f);
            N = norm(mk(-dzdu, -dzdv, 1.0f) * ((k & 1) ? -1.0f : 1.0f));
        });
    }
    // vases: glass and polished metal
    for (int k = 0; k < 4; k++) {
        const float vx = -13.5f + k * 9.0f, vz = (k & 1) ? 2.5f : -2.5f;
        patch(m, T(64), T(48), M_VASE0 + k, 2.0f, 2.0f, true, [&](float u, float v, V & P, V & N) {
            const float a = 2 * PI * u; const float t = v;
            const float r = 0.25f + 0.55f * sinf(PI * (0.15f + 0.8f * t)) * (1.0f - 0.45f * t);
            P = mk(vx + r * cosf(a), 0.05f + 2.2f * t, vz + r * sinf(a));
            const float e = 0.01f, t1 = t + e; const float r1 = 0.25f + 0.55f * sinf(PI * (0.15f + 0.8f * t1)) * (1.0f - 0.45f * t1);
            const float dr = (r1 - r) / (2.2f * e);
            N = norm(mk(cosf(a), -dr, sinf(a)));
        });
    }
    // rough statues: noisy spheres on plinths
    for (int k = 0; k < 4; k++) {
        const float sx = -18.0f + k * 12.0f, sz = (k & 1) ? -3.5f : 3.5f;
        patch(m, T(128), T(96), M_STATUE0 + k, 3.0f, 3.0f, true, [&](float u, float v, V & P, V & N) {
            const float a = 2 * PI * u, b = PI * (v - 0.5f);
            const V d = mk(cosf(a) * cosf(b), sinf(b), sinf(a) * cosf(b));
            const float r = 0.9f + 0.18f * vnoise(6.0f * u * 3.0f + k * 11.0f, 6.0f * v * 3.0f, seed + 31) + 0.05f * vnoise(40.0f * u, 40.0f * v, seed + 33);
            P = mk(sx, 2.0f, sz) + d * r; N = d;
        });
        patch(m, 4, 2, M_TRIM + 1, 1.0f, 1.0f, true, [&](float u, float v, V & P, V & N) {       // plinth (large triangles)
            const float a = 2 * PI * u + 0.25f * PI;
            P = mk(sx + 0.9f * cosf(a), 1.1f * v, sz + 0.9f * sinf(a)); N = norm(mk(cosf(a), 0, sinf(a)));
        });
    }
    // partial roof with a skylight slot (lets the sun and the sky in)
    for (int side = 0; side < 2; side++) {
        const float z0 = side ? 4.0f : -HZ, z1 = side ? HZ : -4.0f;
        patch(m, T(40), T(8), M_TRIM + 2, 12.0f, 3.0f, true, [&](float u, float v, V & P, V & N) {
            P = mk(-HX + 2 * HX * u, HY, z0 + (z1 - z0) * v); N = mk(0, -1, 0);
        });
    }

    const int n = (int)m.mat.size();
    out->triangle_count = n; out->material_count = M_COUNT;
    out->positions = (float *)malloc(sizeof(float) * 9 * (size_t)n);
    out->normals   = (float *)malloc(sizeof(float) * 9 * (size_t)n);
    out->texcoords = (float *)malloc(sizeof(float) * 6 * (size_t)n);
    out->material_ids = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
    if (!out->positions || !out->normals || !out->texcoords || !out->material_ids) return RTX_ERR_OOM;
    memcpy(out->positions, m.pos.data(), sizeof(float) * 9 * (size_t)n);
    memcpy(out->normals, m.nrm.data(), sizeof(float) * 9 * (size_t)n);
    memcpy(out->texcoords, m.uv.data(), sizeof(float) * 6 * (size_t)n);
    memcpy(out->material_ids, m.mat.data(), sizeof(int32_t) * (size_t)n);
    return RTX_OK;
}

extern "C" int rtxh_mesh_free(rtxh_mesh * m) {
    if (!m) return RTX_ERR_INVALID_ARG;
    free(m->positions); free(m->normals); free(m->texcoords); free(m->material_ids);
    memset(m, 0, sizeof(*m));
    return RTX_OK;
}

// =================================================================================================
// `<mesh>.obj.bvh` cache files, BottomLevelBVH::save_to_disk / load_from_disk (BottomLevelBVH.cpp:149-192):
//   int triangle_count; TriangleHot[n]; TriangleCold[n]; int node_count; BVHNode[node_count]; int index_count; int[index_count]
// The record layouts are the C ABI's, so the arrays are handed over as they are; BottomLevelBVH::flatten (:196-212) is the caller's gather.
extern "C" int rtxh_bvh_cache_load(const char * path, rtxh_bvh_cache * out) {
    if (!path || !out) return RTX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    FILE * f = fopen(path, "rb");
    if (!f) return RTX_ERR_STATE;
    fseek(f, 0, SEEK_END); const long size = ftell(f); fseek(f, 0, SEEK_SET);
    auto fail = [&](int rc) { fclose(f); rtxh_bvh_cache_free(out); return rc; };
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n <= 0 || (long long)n * 100 + 12 > size) return fail(RTX_ERR_INVALID_ARG);
    out->triangle_count = n;
    out->hot = (rtx_triangle_hot *)malloc(sizeof(rtx_triangle_hot) * (size_t)n);
    out->cold = (rtx_triangle_cold *)malloc(sizeof(rtx_triangle_cold) * (size_t)n);
    if (!out->hot || !out->cold) return fail(RTX_ERR_OOM);
    if (fread(out->hot, sizeof(rtx_triangle_hot), n, f) != (size_t)n || fread(out->cold, sizeof(rtx_triangle_cold), n, f) != (size_t)n) return fail(RTX_ERR_INVALID_ARG);
    int32_t nodes = 0;
    if (fread(&nodes, 4, 1, f) != 1 || nodes <= 0 || (long long)nodes * 32 > size) return fail(RTX_ERR_INVALID_ARG);
    out->node_count = nodes;
    out->nodes = (rtx_bvh_node *)malloc(sizeof(rtx_bvh_node) * (size_t)nodes);
    if (!out->nodes) return fail(RTX_ERR_OOM);
    if (fread(out->nodes, sizeof(rtx_bvh_node), nodes, f) != (size_t)nodes) return fail(RTX_ERR_INVALID_ARG);
    int32_t idx = 0;
    if (fread(&idx, 4, 1, f) != 1 || idx <= 0 || (long long)idx * 4 > size) return fail(RTX_ERR_INVALID_ARG);
    out->index_count = idx;
    out->indices = (int32_t *)malloc(4 * (size_t)idx);
    if (!out->indices) return fail(RTX_ERR_OOM);
    if (fread(out->indices, 4, idx, f) != (size_t)idx) return fail(RTX_ERR_INVALID_ARG);
    for (int i = 0; i < idx; i++) if (out->indices[i] < 0 || out->indices[i] >= n) return fail(RTX_ERR_INVALID_ARG);
    if (ftell(f) != size) return fail(RTX_ERR_INVALID_ARG);          // trailing bytes: not a cache file of this layout
    fclose(f);
    return RTX_OK;
}

extern "C" int rtxh_bvh_cache_save(const char * path, const rtxh_bvh_cache * c) {
    if (!path || !c || c->triangle_count <= 0 || c->node_count <= 0 || c->index_count <= 0 || !c->hot || !c->cold || !c->nodes || !c->indices) return RTX_ERR_INVALID_ARG;
    FILE * f = fopen(path, "wb");
    if (!f) return RTX_ERR_STATE;
    bool ok = fwrite(&c->triangle_count, 4, 1, f) == 1
           && fwrite(c->hot, sizeof(rtx_triangle_hot), c->triangle_count, f) == (size_t)c->triangle_count
           && fwrite(c->cold, sizeof(rtx_triangle_cold), c->triangle_count, f) == (size_t)c->triangle_count
           && fwrite(&c->node_count, 4, 1, f) == 1 && fwrite(c->nodes, sizeof(rtx_bvh_node), c->node_count, f) == (size_t)c->node_count
           && fwrite(&c->index_count, 4, 1, f) == 1 && fwrite(c->indices, 4, c->index_count, f) == (size_t)c->index_count;
    ok = (fclose(f) == 0) && ok;
    return ok ? RTX_OK : RTX_ERR_STATE;
}

extern "C" int rtxh_bvh_cache_free(rtxh_bvh_cache * c) {
    if (!c) return RTX_ERR_INVALID_ARG;
    free(c->hot); free(c->cold); free(c->nodes); free(c->indices);
    memset(c, 0, sizeof(*c));
    return RTX_OK;
}

// ---- rtx_blas_vertex_normals on the host: csrc/rtx_normals_math.h driven the OTHER way round — the device gathers per vertex through a sorted
// inverted index, this is the plain scatter loop over triangles and corners.  Both add a vertex's face vectors in ascending corner order.
extern "C" int rtxh_vertex_normals(const float * positions, const int32_t * indices, int32_t triangle_count, int32_t vertex_count, float * normals_out) {
    if (!positions || !indices || !normals_out || triangle_count < 1 || vertex_count < 1) return RTX_ERR_INVALID_ARG;
    std::vector<float> acc((size_t)3 * vertex_count, 0.0f);
    for (int32_t t = 0; t < triangle_count; t++) {
        const int32_t * const tri = indices + 3 * (size_t)t;
        if (!rtxn::valid_triangle(tri[0], tri[1], tri[2], vertex_count)) continue;
        float f[3];
        rtxn::face_vector(positions + 3 * (size_t)tri[0], positions + 3 * (size_t)tri[1], positions + 3 * (size_t)tri[2], f);
        for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) acc[3 * (size_t)tri[k] + a] += f[a];
    }
    for (int32_t v = 0; v < vertex_count; v++) rtxn::normalise(&acc[3 * (size_t)v], normals_out + 3 * (size_t)v);
    return RTX_OK;
}

// ---- rtx_blas_pseudonormals on the host: csrc/rtx_side_math.h driven the OTHER way round — the device gathers per vertex and per slot edge
// through the sorted inverted index, this is the plain loop over triangles and corners: the vertex sums are scattered, and the corner lists an
// edge walks are filled by counting, both in ascending corner order.
extern "C" int rtxh_blas_pseudonormals(const float * positions, const int32_t * indices, int32_t triangle_count, int32_t vertex_count,
                                       const int32_t * slot_vertices, int32_t slots, float * vert_out, float * edge_out) {
    if (!positions || !indices || triangle_count < 1 || vertex_count < 1 || slots < 0 || (slots && edge_out && !slot_vertices) || (!vert_out && !edge_out)) return RTX_ERR_INVALID_ARG;
    const size_t T = (size_t)triangle_count, V = (size_t)vertex_count;
    std::vector<float> rec(16 * T);
    for (size_t t = 0; t < T; t++) rtxsd::triangle_record(indices, positions, (uint32_t)t, vertex_count, &rec[16 * t]);
    if (vert_out) {
        std::vector<float> acc(3 * V, 0.0f);
        for (size_t t = 0; t < T; t++) {
            const int32_t * const tri = indices + 3 * t;
            if (!rtxn::valid_triangle(tri[0], tri[1], tri[2], vertex_count)) continue;
            for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) acc[3 * (size_t)tri[k] + a] += rec[16 * t + 4 + 4 * k + a];
        }
        for (size_t v = 0; v < V; v++) rtxsd::finish_sum(&acc[3 * v], vert_out + 4 * v);
    }
    if (edge_out && slots) {
        std::vector<uint32_t> first(V + 1, 0u);                      // the corner lists: triangles in ascending corner order
        for (size_t t = 0; t < T; t++) { const int32_t * const tri = indices + 3 * t; if (rtxn::valid_triangle(tri[0], tri[1], tri[2], vertex_count)) for (int k = 0; k < 3; k++) first[(size_t)tri[k] + 1]++; }
        for (size_t v = 0; v < V; v++) first[v + 1] += first[v];
        std::vector<uint32_t> fill(first.begin(), first.end() - 1), list(first[V]);
        for (size_t t = 0; t < T; t++) { const int32_t * const tri = indices + 3 * t; if (rtxn::valid_triangle(tri[0], tri[1], tri[2], vertex_count)) for (int k = 0; k < 3; k++) list[fill[tri[k]]++] = (uint32_t)t; }
        for (size_t e = 0; e < 3 * (size_t)slots; e++) {
            int32_t x, y;
            rtxsd::edge_vertices(slot_vertices + 3 * (e / 3), (int)(e % 3), x, y);
            float s[3] = { 0.0f, 0.0f, 0.0f };
            if (x >= 0 && x < vertex_count && y >= 0 && y < vertex_count)
                for (uint32_t k = first[x]; k < first[x + 1]; k++) {
                    const uint32_t t = list[k];
                    if (rtxsd::has_vertex(indices + 3 * (size_t)t, y)) for (int a = 0; a < 3; a++) s[a] += rec[16 * (size_t)t + a];
                }
            rtxsd::finish_sum(s, edge_out + 4 * e);
        }
    }
    return RTX_OK;
}

// ---- rtx_refit_blas on the host: csrc/rtx_refit_math.h, the code the kernels run, driven sequentially -----------------------------------
extern "C" int rtxh_blas_refit(rtx_bvh_node * nodes, int32_t node_count, const int32_t * slot_vertices, int32_t triangle_count,
                               const float * positions, const float * normals, int32_t vertex_count,
                               rtx_triangle_hot * hot_out, rtx_triangle_cold * cold) {
    if (!nodes || node_count < 1 || triangle_count < 0 || vertex_count < 0 || (triangle_count > 0 && (!slot_vertices || !positions || !hot_out))) return RTX_ERR_INVALID_ARG;
    if (normals && triangle_count > 0 && !cold) return RTX_ERR_INVALID_ARG;
    for (int64_t k = 0; k < 3 * (int64_t)triangle_count; k++) if (slot_vertices[k] < 0 || slot_vertices[k] >= vertex_count) return RTX_ERR_INVALID_ARG;
    // the reachable nodes in pre-order; every leaf range inside the slots, every child pair inside the nodes, no node reachable twice
    std::vector<int> order, stack(1, 0);
    std::vector<unsigned char> seen((size_t)node_count, 0);
    while (!stack.empty()) {
        const int i = stack.back(); stack.pop_back();
        if (seen[i]) return RTX_ERR_INVALID_ARG;
        seen[i] = 1; order.push_back(i);
        const int cnt = nodes[i].count & 0x3fffffff, f = nodes[i].left_or_first;
        if (cnt > 0) { if (f < 0 || (int64_t)f + cnt > triangle_count) return RTX_ERR_INVALID_ARG; }
        else { if (f < 0 || f + 1 >= node_count) return RTX_ERR_INVALID_ARG; stack.push_back(f); stack.push_back(f + 1); }
    }
    for (int k = 0; k < triangle_count; k++) {
        const float * v0 = positions + 3 * (size_t)slot_vertices[3 * k], * v1 = positions + 3 * (size_t)slot_vertices[3 * k + 1], * v2 = positions + 3 * (size_t)slot_vertices[3 * k + 2];
        memcpy(hot_out[k].position_0, v0, 12);
        rtxr::edges(v0, v1, v2, hot_out[k].position_edge_1, hot_out[k].position_edge_2);
        if (normals) {
            const float * n0 = normals + 3 * (size_t)slot_vertices[3 * k], * n1 = normals + 3 * (size_t)slot_vertices[3 * k + 1], * n2 = normals + 3 * (size_t)slot_vertices[3 * k + 2];
            memcpy(cold[k].normal_0, n0, 12);
            rtxr::edges(n0, n1, n2, cold[k].normal_edge_1, cold[k].normal_edge_2);
        }
    }
    auto load = [&](int i) { rtxu::Box b; memcpy(b.mn, nodes[i].aabb_min, 12); memcpy(b.mx, nodes[i].aabb_max, 12); return b; };
    for (size_t o = order.size(); o-- > 0; ) {                      // children before parents
        const int i = order[o], cnt = nodes[i].count & 0x3fffffff, f = nodes[i].left_or_first;
        rtxu::Box b;
        if (cnt > 0) {
            b = rtxr::empty_box();
            for (int k = f; k < f + cnt; k++)
                rtxr::expand_box(b, rtxr::triangle_box(positions + 3 * (size_t)slot_vertices[3 * k], positions + 3 * (size_t)slot_vertices[3 * k + 1], positions + 3 * (size_t)slot_vertices[3 * k + 2]));
            rtxr::finish_leaf(b);
        } else b = rtxr::join_children(load(f), load(f + 1));
        memcpy(nodes[i].aabb_min, b.mn, 12); memcpy(nodes[i].aabb_max, b.mx, 12);
    }
    return RTX_OK;
}

// ---- rtx_build_blas on the host: csrc/rtx_build_math.h, the code the kernels run, driven sequentially -----------------------------------
extern "C" int32_t rtxh_blas_balanced_node_count(int32_t n) { return n < 1 || n >= RTX_BUILD_MAX_TRIANGLES ? 0 : rtxb::tree_node_count(n); }
extern "C" int32_t rtxh_blas_balanced_inner_depth(int32_t n) { return n < 1 || n >= RTX_BUILD_MAX_TRIANGLES ? -1 : rtxb::tree_inner_depth(n); }

extern "C" int rtxh_blas_build_balanced(const float * positions, const int32_t * indices, const float * normals, const float * texcoords,
                                        const int32_t * material_ids, int32_t T, int32_t V,
                                        rtx_bvh_node * nodes_out, int32_t * node_count_out, rtx_triangle_hot * hot_out, rtx_triangle_cold * cold_out,
                                        int32_t * order_out, int32_t * slot_vertices_out) {
    if (T < 1 || V < 1 || !positions || !indices || !normals || !nodes_out || !node_count_out || !hot_out || !cold_out || !order_out || !slot_vertices_out) return RTX_ERR_INVALID_ARG;
    if (material_ids) for (int i = 0; i < T; i++) if (material_ids[i] < 0) return RTX_ERR_INVALID_ARG;
    if (T >= RTX_BUILD_MAX_TRIANGLES) return RTX_ERR_LIMIT;
    auto vertex = [&](const float * v, int32_t i) { return v + 3 * (size_t)i; };
    // k_build_bounds
    std::vector<unsigned char> ok((size_t)T, 0);
    std::vector<float> centres((size_t)3 * T, 0.0f);
    uint32_t bounds[6] = { RTXU_KEY_LO_INIT, RTXU_KEY_LO_INIT, RTXU_KEY_LO_INIT, RTXU_KEY_HI_INIT, RTXU_KEY_HI_INIT, RTXU_KEY_HI_INIT };
    for (int t = 0; t < T; t++) {
        const int32_t i0 = indices[3 * (size_t)t], i1 = indices[3 * (size_t)t + 1], i2 = indices[3 * (size_t)t + 2];
        if (!rtxb::indices_valid(i0, i1, i2, V)) continue;
        float * c = &centres[3 * (size_t)t];
        if (!rtxb::centre(vertex(positions, i0), vertex(positions, i1), vertex(positions, i2), c)) { c[0] = c[1] = c[2] = 0.0f; continue; }
        ok[t] = 1;
        for (int a = 0; a < 3; a++) { const uint32_t k = rtxu::ordered_key(c[a]); if (k < bounds[a]) bounds[a] = k; if (k > bounds[3 + a]) bounds[3 + a] = k; }
    }
    // k_build_keys + the sort: the keys are distinct (the index is part of them), so there is one result
    std::vector<uint64_t> keys((size_t)T);
    for (int t = 0; t < T; t++) keys[t] = rtxb::sort_key(&centres[3 * (size_t)t], bounds, (uint32_t)t, ok[t] != 0);
    std::sort(keys.begin(), keys.end());
    // k_build_scatter
    for (int k = 0; k < T; k++) {
        const int t = (int)(keys[k] & (((uint64_t)1 << RTXB_INDEX_BITS) - 1));
        const int32_t i0 = indices[3 * (size_t)t], i1 = indices[3 * (size_t)t + 1], i2 = indices[3 * (size_t)t + 2];
        const bool valid = rtxb::indices_valid(i0, i1, i2, V);
        int32_t * sv = slot_vertices_out + 3 * (size_t)k;
        sv[0] = valid ? i0 : -1; sv[1] = valid ? i1 : -1; sv[2] = valid ? i2 : -1;
        order_out[k] = t;
        memset(&cold_out[k], 0, sizeof(rtx_triangle_cold));
        cold_out[k].material_id = material_ids ? material_ids[t] : 0;
        if (!valid) {
            const uint32_t q = RTXB_NAN_BITS;
            float * h = hot_out[k].position_0;                             // nine floats in a row
            for (int a = 0; a < 9; a++) memcpy(h + a, &q, 4);
            continue;
        }
        memcpy(hot_out[k].position_0, vertex(positions, i0), 12);
        rtxr::edges(vertex(positions, i0), vertex(positions, i1), vertex(positions, i2), hot_out[k].position_edge_1, hot_out[k].position_edge_2);
        memcpy(cold_out[k].normal_0, vertex(normals, i0), 12);
        rtxr::edges(vertex(normals, i0), vertex(normals, i1), vertex(normals, i2), cold_out[k].normal_edge_1, cold_out[k].normal_edge_2);
        if (texcoords) for (int a = 0; a < 2; a++) {
            const float u0 = texcoords[2 * (size_t)i0 + a];
            cold_out[k].tex_coord_0[a] = u0;
            cold_out[k].tex_coord_edge_1[a] = texcoords[2 * (size_t)i1 + a] - u0;
            cold_out[k].tex_coord_edge_2[a] = texcoords[2 * (size_t)i2 + a] - u0;
        }
    }
    // the topology, and the boxes level by level from the deepest (k_build_level / k_build_top)
    const int levels = rtxb::tree_levels(T), slots = rtxb::tree_node_count(T);
    memset(nodes_out, 0, sizeof(rtx_bvh_node) * (size_t)slots);
    auto load = [&](int i) { rtxu::Box b; memcpy(b.mn, nodes_out[i].aabb_min, 12); memcpy(b.mx, nodes_out[i].aabb_max, 12); return b; };
    for (int d = levels; d >= 0; d--)
        for (int j = 0; j < (1 << d); j++) {
            int first;
            const int cnt = rtxb::node_range(T, d, j, &first), slot = rtxu::node_slot(d, j);
            if (cnt == 0) continue;
            rtxu::Box b;
            if (cnt <= RTX_BUILD_LEAF_MAX) {
                b = rtxr::empty_box();
                for (int k = first; k < first + cnt; k++) {
                    const int32_t * sv = slot_vertices_out + 3 * (size_t)k;
                    if (sv[0] < 0) continue;
                    rtxr::expand_box(b, rtxr::triangle_box(vertex(positions, sv[0]), vertex(positions, sv[1]), vertex(positions, sv[2])));
                }
                rtxr::finish_leaf(b);
                nodes_out[slot].left_or_first = first; nodes_out[slot].count = cnt;
            } else {
                const int left = (2 << d) | (2 * j);
                const rtxu::Box l = load(left), r = load(left + 1);
                b = rtxr::join_children(l, r);
                nodes_out[slot].left_or_first = left; nodes_out[slot].count = (int32_t)((uint32_t)rtxb::join_axis(l, r) << 30);
            }
            memcpy(nodes_out[slot].aabb_min, b.mn, 12); memcpy(nodes_out[slot].aabb_max, b.mx, 12);
        }
    *node_count_out = slots;
    return RTX_OK;
}
