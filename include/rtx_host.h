/*
 * rtx_host.h — C ABI of librtx_host.so: the host-side callers of the render path.
 *
 * CPU-only code that prepares what include/rtx.h consumes, i.e. the reference's per-frame
 * Scene::update (Scene.cpp:139-171) and its load-time BottomLevelBVH construction.  Nothing here
 * runs on the GPU and nothing here renders; the render path itself is librtx_hip.so.
 *
 *   rtxh_camera_basis        Camera::resize + Camera::update basis       Camera.cpp:5-16,44-47
 *   rtxh_camera_update       Camera::update keyboard movement             Camera.cpp:18-39
 *   rtxh_instance_update     Mesh::update                                 Mesh.cpp:9-15
 *                            (Transform::calc_world_matrix Transform.h:13-43, AABB::transform
 *                             AABB.cpp:55-73, Matrix4::invert Matrix4.h:88-138)
 *   rtxh_plane_update        Plane::update                                Plane.cpp:3-11
 *   rtxh_quaternion_axis_angle  Quaternion::axis_angle                     Quaternion.h:26-36
 *   rtxh_scene_update        Scene::update's tail: all Mesh::update + TLAS rebuild   Scene.cpp:166-170
 *   rtxh_scene_dynamic_animate  SCENE_DYNAMIC's animation                   Scene.cpp:141-155
 *   rtxh_tlas_*              TopLevelBVH::init / build_bvh                TopLevelBVH.cpp:5-45
 *                            (BVHBuilders::build_bvh<Mesh> BVHBuilders.h:8-46,
 *                             BVHPartitions::{calculate_bounds,partition_sah,split_indices})
 *   rtxh_tlas_build_balanced this repo's OWN TLAS builder: the tree rtx_update_instances builds on the device, from the same
 *                            code (csrc/rtx_update_math.h); rtxh_scene_update_balanced = rtx_update_instances on the host
 *   rtxh_blas_refit          this repo's OWN refit of a flattened BLAS to moved vertices: what rtx_refit_blas leaves on the device,
 *                            from the same code (csrc/rtx_refit_math.h)
 *   rtxh_blas_build_balanced this repo's OWN balanced BLAS of an indexed mesh: the tree rtx_build_blas builds on the device, from the
 *                            same code (csrc/rtx_build_math.h)
 *   rtxh_vertex_normals      this repo's OWN smooth, area-weighted vertex normals of an indexed mesh: what rtx_blas_vertex_normals writes on
 *                            the device, from the same code (csrc/rtx_normals_math.h)
 *   rtxh_blas_build          a BottomLevelBVH for a triangle soup: this repo's OWN binned-SAH
 *                            builder (not the reference's SBVH), output in the
 *                            reference's node convention + flattened leaf order
 *                            (BVHNode.h:10-28, BottomLevelBVH.cpp:196-212)
 *   rtxh_blas_build_reference_bvh   the reference's non-spatial BLAS builder, node for node (BVHBuilders.h:8-46)
 *   rtxh_blas_build_reference_sbvh  the reference's DEFAULT BLAS builder (MESH_ACCELERATOR_SBVH, Config.h:35): spatial
 *                            splits + reference unsplitting, node for node     BVHBuilders.h:48-329, BVHPartitions.h:117-377
 *   rtxh_obj_load            OBJLoader::load_obj / load_mtl                 OBJLoader.cpp:8-187
 *   rtxh_mtl_load            OBJLoader::load_mtl alone                       OBJLoader.cpp:43-68
 *   rtxh_bvh_cache_*         BottomLevelBVH::save_to_disk / load_from_disk   BottomLevelBVH.cpp:149-192
 *   rtxh_texture_mips        Texture::load's box-filter mip chain          Texture.cpp:76-117
 *   rtxh_query_sort_order    the order RTX_QUERY_SORT traces query rows in, from the same code (csrc/rtx_query_sort_math.h)
 *   rtxh_query_nearest       rtx_query_nearest on the host: the walk and the arithmetic of csrc/rtx_nearest_math.h over plain arrays;
 *                            rtxh_query_nearest_exhaustive the same candidate functions over every primitive, without a tree
 *   rtxh_query_sweep         rtx_query_sweep on the host: the walk and the arithmetic of csrc/rtx_sweep_math.h over the same arrays;
 *   rtxh_query_sweep_box     rtx_query_sweep_box on the host: the walk and the arithmetic of csrc/rtx_boxsweep_math.h over the same arrays;
 *                            rtxh_query_sweep_box_exhaustive the same candidate functions over every primitive, without a node test
 *   rtxh_query_*_filtered    the three walk queries under object masks (rtx_query_*_filtered), and their exhaustive searches over the visible primitives
 *   rtxh_blas_pseudonormals  rtx_blas_pseudonormals on the host: the angle-weighted pseudonormal tables of csrc/rtx_side_math.h as a plain loop;
 *   rtxh_query_signed_distance  rtx_query_signed_distance on the host (and its _exhaustive / _filtered forms): rtxh_query_nearest with the sign
 *   rtxh_query_hits          rtx_query_hits on the host: the walk and the arithmetic of csrc/rtx_hits_math.h over the same arrays;
 *                            rtxh_query_hits_exhaustive the same hit tests over every primitive, without a box test
 *   rtxh_texture_load        Texture::load: PNG / TGA file -> linear float3 texels + mips   Texture.cpp:30-129
 *   rtxh_image_load          the stbi_load(..., STBI_rgb_alpha) call inside it  Texture.cpp:40
 *   rtxh_sky_load            Sky::Sky: raw float3 angular-map probe file         Sky.cpp:8-26
 *   rtxh_atrium_*            seeded procedural stand-in for the absent Sponza mesh
 */
#ifndef RTX_HOST_H
#define RTX_HOST_H

#include <stdint.h>
#include "rtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* position[3], rotation quaternion (x,y,z,w), fov in radians -> rtx_camera */
int rtxh_camera_basis(int32_t width, int32_t height, float fov, const float position[3], const float rotation[4], rtx_camera * out);

/* Mesh::update: fills out->world / world_inv (blas_id untouched) and the world-space AABB of the instance */
int rtxh_instance_update(const float position[3], const float rotation[4], const float blas_root_min[3], const float blas_root_max[3],
                         rtx_instance * out, float out_aabb_min[3], float out_aabb_max[3]);

/* Quaternion::axis_angle (Quaternion.h:26-36) with the host libm's sinf / cosf, as the reference evaluates it */
int rtxh_quaternion_axis_angle(const float axis[3], float angle, float out[4]);

int rtxh_plane_update(const float position[3], const float rotation[4], int32_t material_id, rtx_plane * out);

/* Persistent TLAS builder (keeps the three index arrays across frames like TopLevelBVH does). */
typedef struct rtxh_tlas rtxh_tlas;
int rtxh_tlas_create(int32_t instance_count, rtxh_tlas ** out);
int rtxh_tlas_destroy(rtxh_tlas * t);
/* positions: n*3 (Mesh::get_position = transform.position), aabbs: n*6 (min,max).  nodes_out holds
 * 2*n entries, indices_out n entries; *node_count_out receives TopLevelBVH::node_count.          */
int rtxh_tlas_build(rtxh_tlas * t, const float * positions, const float * aabbs,
                    rtx_bvh_node * nodes_out, int32_t * indices_out, int32_t * node_count_out);

/* The balanced TLAS of rtx_update_instances (include/rtx.h), built on the host by the code the kernels run (csrc/rtx_update_math.h): the
 * instances sorted by (box finite?, 30-bit Morton code of their position over the bounds of all finite positions, instance index) — an
 * instance whose box has a NaN or infinite component sorts first, so that a NaN inner box never covers a finite instance —, an implicit heap over
 * the sorted range — node (d, j) covers sorted slots [j*n >> d, (j+1)*n >> d), is a leaf when that is one slot and is stored at index
 * 2^d + j (root at 0, index 1 unused, children adjacent) — and boxes bottom-up: a leaf's box is its instance's after AABB::fix_if_needed
 * (AABB.h:26-32), an inner node's the union of its children's STORED boxes, then fix_if_needed.  `count` of an inner node carries the axis
 * (1..3, bits 30-31) on which the right child's box centre lies furthest beyond the left child's.  Shape, node count and depth depend on n
 * alone; slots that are no node are zero.  Defined for every float input: the indices are always a permutation, every range lies inside the
 * arrays.  O(n log n).  positions n*3, aabbs n*6 (min, max); nodes_out holds rtxh_tlas_balanced_node_count(n) entries, indices_out n.
 * 1 <= n <= 65 536 (RTX_ERR_LIMIT above).                                                                                                  */
/* The rigid rule of the length queries (include/rtx.h, rtx_query_nearest: Limits), the one definition rtx_set_frame compiles: 1 when for
 * every instance the linear parts R of world and world_inv have every |(R.R^T - I)ij| <= 2^-12 in fp64, else 0 (a NaN cell: 0; no instances:
 * 1).  deviation_out (may be NULL): the largest such entry over all instances.                                                             */
int rtxh_instances_rigid(const rtx_instance * instances, int32_t instance_count, double * deviation_out);
int32_t rtxh_tlas_balanced_node_count(int32_t instance_count);     /* 2 << ceil(log2 n); 0 for n outside the supported range */
int32_t rtxh_tlas_balanced_inner_depth(int32_t instance_count);    /* depth of the deepest inner node (-1 for one instance): ceil(log2 n) - 1 */
int rtxh_tlas_build_balanced(int32_t instance_count, const float * positions, const float * aabbs,
                             rtx_bvh_node * nodes_out, int32_t * indices_out, int32_t * node_count_out);
/* rtxh_scene_update with that builder and the kernels' restatement of Mesh::update: what rtx_update_instances leaves on the device.  The
 * instance records equal rtxh_scene_update's bit for bit.                                                                                  */
int rtxh_scene_update_balanced(int32_t instance_count, const float * positions, const float * rotations, const int32_t * blas_ids,
                               const float * blas_root_aabbs, rtx_instance * instances_out, rtx_bvh_node * tlas_nodes_out,
                               int32_t * tlas_indices_out, int32_t * tlas_node_count_out);

/* Triangle soup -> flattened BLAS.  positions: n*9 floats (p0,p1,p2).  nodes_out must hold 2*n
 * entries, order_out n entries: order_out[k] = source triangle stored at flattened slot k.       */
int rtxh_blas_build(const float * positions, int32_t triangle_count, int32_t bins,
                    rtx_bvh_node * nodes_out, int32_t * node_count_out, int32_t * order_out);

/* The reference's NON-spatial builder (MESH_ACCELERATOR_BVH, BottomLevelBVH::build_bvh BottomLevelBVH.cpp:72-106 over
 * BVHBuilders::build_bvh<Triangle> BVHBuilders.h:8-46): three index lists sorted by triangle centroid
 * (Triangle::get_position, Triangle.h:22-24), full-sweep SAH, leaves below 3 triangles.  Same arguments as rtxh_blas_build;
 * produces the reference's node array and leaf order for that build mode (checked against a reference dump).            */
int rtxh_blas_build_reference_bvh(const float * positions, int32_t triangle_count,
                                  rtx_bvh_node * nodes_out, int32_t * node_count_out, int32_t * order_out);

/* The reference's SBVH builder (MESH_ACCELERATOR_SBVH, the shipped default: BottomLevelBVH::build_sbvh BottomLevelBVH.cpp:108-147 over
 * BVHBuilders::build_sbvh BVHBuilders.h:48-329, BVHPartitions::partition_object / partition_spatial BVHPartitions.h:117-377).
 * A triangle may be referenced from several leaves, so the flattened order is longer than the mesh: order_out receives
 * *order_count_out (>= triangle_count) source-triangle ids, nodes_out *node_count_out nodes.  The reference sizes both
 * arrays at 2 * triangle_count and overruns them beyond that; here a mesh that needs more than the capacities given returns
 * RTX_ERR_LIMIT (call again with larger arrays).  Output checked bit for bit against trees built by the reference.            */
int rtxh_blas_build_reference_sbvh(const float * positions, int32_t triangle_count,
                                   rtx_bvh_node * nodes_out, int32_t node_capacity, int32_t * node_count_out,
                                   int32_t * order_out, int32_t order_capacity, int32_t * order_count_out);

/* rtx_refit_blas (include/rtx.h) on the host, by the code the kernels run (csrc/rtx_refit_math.h): keeps the topology of a flattened BLAS
 * (left_or_first, count and every unreachable node slot are not touched) and rewrites, for vertices that moved,
 *   hot_out[k]   position_0, position_edge_1 = p1 - p0, position_edge_2 = p2 - p0 of slot k, p_c = positions[slot_vertices[3k + c]];
 *   cold[k]      with normals != NULL the three normal fields the same way (texture coordinates and material ids stay); NULL: untouched;
 *   nodes[i]     the box of every node reachable from the root, bottom-up: a triangle's box is AABB::from_points over its vertices, then
 *                AABB::fix_if_needed (Triangle.h:17-22); a leaf's the union of its triangles' boxes in slot order, then fix_if_needed; an
 *                inner node's the union of its children's STORED boxes, left first, then fix_if_needed (BVHPartitions.h:11-23).
 * Any float is a legal coordinate: a NaN or infinite component takes no part in a box, an axis on which a leaf has no finite component takes
 * [+0, +0] before the fix.  So every reachable box is finite, min <= max, and children are nested in their parents, whatever the input; a
 * triangle with a non-finite vertex may become invisible.  slot_vertices: 3 vertex indices per flattened slot (slot k = order_out[k] of the
 * builders: 3 * order_out[k] + c for a soup; duplicated SBVH references repeat indices).  The output handed to rtx_upload_blas is by
 * definition what rtx_refit_blas leaves on the device.  RTX_ERR_INVALID_ARG: null pointer, an index outside [0, vertex_count), a tree whose
 * reachable part leaves the arrays or is no tree.                                                                                        */
int rtxh_blas_refit(rtx_bvh_node * nodes, int32_t node_count, const int32_t * slot_vertices, int32_t triangle_count,
                    const float * positions, const float * normals_or_null, int32_t vertex_count,
                    rtx_triangle_hot * hot_out, rtx_triangle_cold * cold);

/* rtx_alloc_blas + rtx_build_blas (include/rtx.h) on the host, by the code the kernels run (csrc/rtx_build_math.h): this repo's OWN balanced
 * BLAS over an indexed mesh — positions V*3, indices T*3, normals V*3, texcoords V*2 or NULL (zeros), material_ids T local ids or NULL (0).
 *   validity   a triangle with an index outside [0, vertex_count) is INVALID (-1 is the documented padding): nothing is read through its
 *              indices, its hot record is nine quiet NaNs (0x7fc00000), its cold record zero but for the material id, its slot_vertices
 *              entry -1 -1 -1, and it takes no part in any box;
 *   order      triangles sorted by (valid and box finite?, 30-bit Morton code of the centre 0.5 min + 0.5 max of their box over the bounds of
 *              all such centres, source triangle index): triangles without the bit come first in index order.  order_out[k] = the source
 *              triangle stored in flattened slot k, slot_vertices_out[3k + c] its vertex indices (the table rtx_refit_blas goes by);
 *   shape      an implicit heap: node (d, j) covers slots [j*T >> d, (j+1)*T >> d), is a leaf when that is at most 4 slots
 *              (RTX_BUILD_LEAF_MAX) and is stored at index 2^d + j — root at 0, index 1 unused, children adjacent, `left` even.  Shape, node
 *              count and depth depend on T alone; slots that are no node are zero bytes;
 *   boxes      rtxh_blas_refit's rules exactly (a leaf whose triangles are all invalid takes that rule's [+0, +0] box before the fix);
 *              rtxh_blas_refit on the output with the same vertices returns the same boxes;
 *   axis       bits 30-31 of an inner node's `count`: the axis on which the right child's box centre lies furthest beyond the left child's.
 * Any float is a legal coordinate.  nodes_out holds rtxh_blas_balanced_node_count(T) entries, hot_out / cold_out / order_out T,
 * slot_vertices_out 3T.  RTX_ERR_INVALID_ARG: null pointer, T < 1, V < 1, a negative material id; RTX_ERR_LIMIT: T >= 2^24.              */
int32_t rtxh_blas_balanced_node_count(int32_t triangle_count);     /* 2 << L, L = the first level with ceil(T / 2^L) <= 4; 0 for T outside the supported range */
int32_t rtxh_blas_balanced_inner_depth(int32_t triangle_count);    /* depth of the deepest inner node: L - 1 (-1: the root is a leaf) */
int rtxh_blas_build_balanced(const float * positions, const int32_t * indices, const float * normals, const float * texcoords_or_null,
                             const int32_t * material_ids_or_null, int32_t triangle_count, int32_t vertex_count,
                             rtx_bvh_node * nodes_out, int32_t * node_count_out, rtx_triangle_hot * hot_out, rtx_triangle_cold * cold_out,
                             int32_t * order_out, int32_t * slot_vertices_out);

/* rtx_blas_vertex_normals (include/rtx.h) on the host, by the code the kernels run (csrc/rtx_normals_math.h): smooth, area-weighted vertex
 * normals of an indexed mesh — positions V*3, indices T*3, normals_out V*3.  Written as the plain scatter loop (over triangles, over corners,
 * acc[v] += f, then normalise), where the device gathers per vertex through a sorted inverted index: the same additions in the same order.
 *   validity   a triangle with an index outside [0, vertex_count) contributes nothing and nothing is read through its indices;
 *   face       f = (p1 - p0) x (p2 - p0); a face vector with a NaN or infinite component counts as (+0, +0, +0);
 *   sum        from (+0, +0, +0), f once per corner c = 3t + k that holds the vertex, in ascending c;
 *   normal     m = max |component| of the sum; zero or not finite: (+0, +0, +0); else a = s / m, n = a / sqrtf(a.x*a.x + (a.y*a.y + a.z*a.z)).
 * Any float is a legal coordinate; no output component is NaN or infinite.  RTX_ERR_INVALID_ARG: null pointer, T < 1, V < 1.              */
int rtxh_vertex_normals(const float * positions, const int32_t * indices, int32_t triangle_count, int32_t vertex_count, float * normals_out);

/* Camera::update's input handling (Camera.cpp:18-39): keys = OR of RTXH_KEY_* held during this frame; position / rotation are
 * updated in place (follow with rtxh_camera_basis for the view pyramid, Camera.cpp:44-47).                                      */
enum { RTXH_KEY_W = 1, RTXH_KEY_A = 2, RTXH_KEY_S = 4, RTXH_KEY_D = 8, RTXH_KEY_LSHIFT = 16, RTXH_KEY_SPACE = 32,
       RTXH_KEY_UP = 64, RTXH_KEY_DOWN = 128, RTXH_KEY_LEFT = 256, RTXH_KEY_RIGHT = 512 };
int rtxh_camera_update(float delta, uint32_t keys, float position[3], float rotation[4]);

/* Scene::update in two calls (Scene.cpp:139-171).  rtxh_scene_dynamic_animate is the animation SCENE_DYNAMIC hard-codes (:141-155,
 * instances 0..5; *time is the function-static `time`); rtxh_scene_update is the common tail (:166-170): Mesh::update for every
 * instance, then the TLAS rebuild.  positions n*3, rotations n*4 (x,y,z,w), blas_root_aabbs: 6 floats (min, max) per BLAS id.        */
int rtxh_scene_dynamic_animate(float delta, float * time, float * positions, float * rotations, int32_t instance_count);
int rtxh_scene_update(rtxh_tlas * tlas, int32_t instance_count, const float * positions, const float * rotations, const int32_t * blas_ids,
                      const float * blas_root_aabbs, rtx_instance * instances_out, rtx_bvh_node * tlas_nodes_out,
                      int32_t * tlas_indices_out, int32_t * tlas_node_count_out);

/* Appends the box-filter mip chain to level 0 (texels_rgb holds w*h float3 on entry and must have
 * room for w*h + w*h/3 + 1 texels); fills desc like Texture::load.  The shape and the filter are
 * the ones rtx_alloc_texture / rtx_update_texture use on the device (csrc/rtx_texmip_math.h), so
 * the limits are theirs too: RTX_ERR_LIMIT for more than RTX_MAX_MIP_LEVELS levels and, since the
 * two share the code, for an image of more texels than the int32_t offsets of rtx_texture_desc
 * hold (such an image without a chain used to return RTX_OK with a 64-bit count).                */
int rtxh_texture_mips(float * texels_rgb, int32_t width, int32_t height, rtx_texture_desc * desc, int64_t * texel_count_out);

/* The order rtx_query_closest / rtx_query_occluded trace n rows in under RTX_QUERY_SORT: rtx_debug_query_order's contract with host memory.
 * rows: n x row_floats floats (6: origin, direction; 7: with a maximum distance).  Per round of at most RTX_QUERY_CHUNK_RAYS rows the bounds
 * of the live rows, the key of every row (csrc/rtx_query_sort_math.h, the code the kernels compile) and a sort of the keys:
 * order_out[first + i] = first + the row in slot i of the round that starts at `first`.  Dead rows (zero direction, a non-finite origin or
 * direction, a NaN maximum distance) come last in row order.  row_floats 4: the points of rtx_query_nearest (x, y, z, maximum distance) — live with
 * finite x, y, z and a maximum distance > 0, sorted by the Morton code of the point alone.  RTX_ERR_INVALID_ARG: a null pointer, n < 1,
 * row_floats other than 4, 6 or 7; RTX_ERR_LIMIT: n beyond INT32_MAX.                                                                 */
int rtxh_query_sort_order(const float * rows, int32_t row_floats, int64_t n, int32_t * order_out);

/* rtx_query_nearest (include/rtx.h) on the host, by the code the kernel runs (csrc/rtx_nearest_math.h, whose header comment is the
 * specification: candidate functions, the order of the walk, the stack count, the accuracy bound).  The scene as plain arrays: what a
 * scene file holds, or what rtx_read_frame_state / rtx_read_blas return, so a device-updated scene can be checked.  points: n x 4 floats
 * (x, y, z, maximum distance); channels and out as for rtx_query_nearest, with host pointers; the answers are the device's bit for bit.
 * stack_max_out (may be NULL): the most stack entries any row held.
 * rtxh_query_nearest_exhaustive: the same candidate functions over every sphere, plane and (instance, slot) without a tree; an exact tie
 * goes to the lowest (kind, object, slot), kinds in the order sphere, plane, triangle.  The walk's distance is never below the exhaustive
 * one and exceeds it by at most rtxh_nearest_distance_bound(S, W) of the exhaustive winner (S = |p_l - p0| + |e1| + |e2|; W = |p| + |p_l|
 * for an instance whose matrix is not the identity, else 0).
 * RTX_ERR_INVALID_ARG: a null scene / points / out, n < 1, channels 0 or outside RTX_QUERY_ALL, a negative count, a count without its
 * array, an instance whose blas_id is outside [0, blas_count); RTX_ERR_LIMIT: a tree deeper than RTX_MAX_STACK entries of the walk; then
 * RTX_ERR_STATE, from the walks of the length queries only (rtxh_query_nearest, _signed_distance, _sweep, _overlap, _overlap_capsule, _sweep_box and their
 * _filtered forms): an instance that rtxh_instances_rigid does not accept, as on the device (include/rtx.h, rtx_query_nearest: Limits).
 * The exhaustive searches prune nothing and answer for any matrix, in local units; so does rtxh_query_hits.                               */
typedef struct rtxh_nearest_blas {
    const rtx_bvh_node * nodes; const rtx_triangle_hot * hot; const rtx_triangle_cold * cold;
    int32_t node_count, triangle_count, material_offset, pad;
} rtxh_nearest_blas;
typedef struct rtxh_nearest_scene {
    const rtx_instance * instances; const rtx_bvh_node * tlas_nodes; const int32_t * tlas_indices; const rtxh_nearest_blas * blas;
    const rtx_sphere * spheres; const rtx_plane * planes;
    int32_t instance_count, tlas_node_count, tlas_index_count, blas_count, sphere_count, plane_count;
} rtxh_nearest_scene;
int rtxh_query_nearest(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out, int32_t * stack_max_out);
int rtxh_query_nearest_exhaustive(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out);
float rtxh_nearest_distance_bound(float local_scale, float world_scale);
/* the candidate functions on their own, for tests that restate them: squared distances (and the triangle's weights) */
float rtxh_nearest_box_d2(const float p[3], const float box_min[3], const float box_max[3]);
float rtxh_nearest_triangle_d2(const float p[3], const rtx_triangle_hot * tri, float uv_out[2]);
float rtxh_nearest_sphere_d2(const float p[3], const rtx_sphere * sphere);
float rtxh_nearest_plane_d2(const float p[3], const rtx_plane * plane);

/* rtx_query_hits (include/rtx.h) on the host, by the code the kernel runs (csrc/rtx_hits_math.h, whose header comment is the specification:
 * what a hit is, the order, the walk and its shrinking bound, what is promised).  The scene is rtxh_nearest_scene; segments: n x 7 floats
 * (origin, direction, max distance); max_hits, channels, out and count_out as for rtx_query_hits, with host pointers and K = max_hits entries
 * per row; the answers are the device's bit for bit.  stack_max_out (may be NULL): the most stack entries any row held.
 * rtxh_query_hits_exhaustive: every sphere, plane and (instance, slot) tested with no box test, the same order rule; count_out is the number
 * of all hits.  Every hit the walk lists is in the exhaustive list with the same bits, and the walk's count never exceeds the exhaustive one.
 * rtxh_hits_margin(kappa, scale): rtxhp::margin, how far tri_test's u, v and t may lie from their exact values (MARGIN in that header).
 * RTX_ERR_INVALID_ARG: the argument rules of rtx_query_hits and rtxh_query_nearest; RTX_ERR_LIMIT: a tree deeper than RTX_MAX_STACK entries. */
int rtxh_query_hits(const rtxh_nearest_scene * scene, const float * segments, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                    int32_t * count_out, int32_t * stack_max_out);
int rtxh_query_hits_exhaustive(const rtxh_nearest_scene * scene, const float * segments, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                               int32_t * count_out);
float rtxh_hits_margin(float kappa, float scale);

/* rtx_query_sweep (include/rtx.h) on the host, by the code the kernel runs (csrc/rtx_sweep_math.h, whose header comment is the specification:
 * candidate functions, the order rule, the walk, the accuracy bound).  The scene is rtxh_nearest_scene; sweeps: n x 8 floats (origin,
 * direction, max distance, radius); channels and out as for rtx_query_sweep, with host pointers; the answers are the device's bit for bit.
 * stack_max_out (may be NULL): the most stack entries any row held.
 * rtxh_query_sweep_exhaustive: the same candidate functions over every sphere, plane and (instance, slot) without a box test, the same order
 * rule.  Within an instance the box tests skip no candidate the exhaustive search would accept; the two still meet the triangles in different
 * orders, and the plane early-out of the triangle test depends on the order within its rounding (ORDER in that header): their t can differ
 * by that much, either way round, and both satisfy the accuracy bound.
 * rtxh_sweep_bound(S, W, T, r): rtxsp::sweep_bound, the bound in distance of ACCURACY in that header (local scale, world scale, length
 * travelled, radius).
 * The candidate functions on their own, for tests that restate them: 1 and *t_out (a triangle's weights in uv_out, the squared distance from
 * the origin in d20_out) when the primitive yields a candidate, else 0.  rtxh_sweep_triangle takes the LOCAL ray and the walk's bound
 * (no answer's d20: the "settled" early-out of the header, which changes no answer, never applies).
 * RTX_ERR_INVALID_ARG, RTX_ERR_STATE and RTX_ERR_LIMIT: as for rtxh_query_nearest.                                                      */
int rtxh_query_sweep(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, uint32_t channels, const rtx_query_buffers * out, int32_t * stack_max_out);
int rtxh_query_sweep_exhaustive(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, uint32_t channels, const rtx_query_buffers * out);
float rtxh_sweep_bound(float local_scale, float world_scale, float travelled, float radius);
int rtxh_sweep_triangle(const float origin[3], const float direction[3], float radius, float bound, const rtx_triangle_hot * tri, float * t_out, float uv_out[2], float * d20_out);
int rtxh_sweep_sphere(const float origin[3], const float direction[3], float radius, const rtx_sphere * sphere, float * t_out, float * d20_out);
int rtxh_sweep_plane(const float origin[3], const float direction[3], float radius, const rtx_plane * plane, float * t_out, float * d20_out);

/* rtx_query_overlap (include/rtx.h) on the host, by the code the kernel runs (csrc/rtx_overlap_math.h, whose header comment is the
 * specification: the row, the triangle / sphere / plane / node tests, the order, the walk, the three forms, the margin, what is promised).  The
 * scene is rtxh_nearest_scene; boxes: n x 10 floats (centre, half extents, quaternion); max_hits, the id arrays, count_out and flags as for
 * rtx_query_overlap, with host pointers and K = max_hits entries per row (RTX_QUERY_SORT is accepted and changes nothing); the answers are the
 * device's bit for bit.  stack_max_out (may be NULL): the most stack entries any row held.
 * rtxh_query_overlap_exhaustive: every sphere, plane and (instance, slot) tested with no node test, the same functions and the same order
 * rule; count_out is the number of all overlaps.  Every overlap the walk lists is in the exhaustive list, and the walk's count never exceeds
 * the exhaustive one.  The _filtered forms take object_masks, row_masks and row_mask as the filtered walk queries below.
 * rtxh_overlap_margin(S, W, kappa): rtxop::margin, how far as a distance the computed triangle test may be from the exact one on an axis of
 * conditioning kappa (MARGIN in that header).
 * RTX_ERR_INVALID_ARG: the argument rules of rtx_query_overlap and rtxh_query_nearest; RTX_ERR_LIMIT: a tree deeper than RTX_MAX_STACK entries;
 * RTX_ERR_STATE: a non-rigid instance (the walk only), as for rtxh_query_nearest. */
int rtxh_query_overlap(const rtxh_nearest_scene * scene, const float * boxes, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                       int32_t * count_out, uint32_t flags, int32_t * stack_max_out);
int rtxh_query_overlap_exhaustive(const rtxh_nearest_scene * scene, const float * boxes, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                  int32_t * count_out, uint32_t flags);
int rtxh_query_overlap_filtered(const rtxh_nearest_scene * scene, const float * boxes, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                int32_t * count_out, uint32_t flags, int32_t * stack_max_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
int rtxh_query_overlap_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * boxes, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                           int32_t * count_out, uint32_t flags, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
float rtxh_overlap_margin(float local_scale, float world_scale, float kappa);

/* rtx_query_overlap_capsule (include/rtx.h) on the host, by the code the kernel runs (csrc/rtx_capsule_math.h, whose header comment is the
 * specification).  As rtxh_query_overlap and its three siblings above, over capsules: n x 7 floats (start point, axis vector, radius); the
 * answers are the device's bit for bit.  rtxh_capsule_margin(S, W, kappa): rtxcp::margin, how far as a distance the computed triangle test
 * may be from the exact one for a sub-test of conditioning kappa (MARGIN in that header).  The error codes are rtxh_query_overlap's. */
int rtxh_query_overlap_capsule(const rtxh_nearest_scene * scene, const float * capsules, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                               int32_t * count_out, uint32_t flags, int32_t * stack_max_out);
int rtxh_query_overlap_capsule_exhaustive(const rtxh_nearest_scene * scene, const float * capsules, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                          int32_t * count_out, uint32_t flags);
int rtxh_query_overlap_capsule_filtered(const rtxh_nearest_scene * scene, const float * capsules, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                        int32_t * count_out, uint32_t flags, int32_t * stack_max_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
int rtxh_query_overlap_capsule_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * capsules, int64_t n, int32_t max_hits, int32_t * object_id_out, int32_t * triangle_id_out,
                                                   int32_t * count_out, uint32_t flags, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
float rtxh_capsule_margin(float local_scale, float world_scale, float kappa);

/* rtx_query_sweep_box (include/rtx.h) on the host, by the code the kernel runs (csrc/rtx_boxsweep_math.h, whose header comment is the
 * specification: candidate functions, the order rule, the walk and its slack, the accuracy bound).  The scene is rtxh_nearest_scene; sweeps:
 * n x 14 floats (centre, direction, max distance, half extents, quaternion); the five outputs as for rtx_query_sweep_box, with host pointers,
 * at least one not NULL; the answers are the device's bit for bit.  Both take the masks of the filtered call: object_masks (M masks or NULL:
 * all ones), row_masks (n masks or NULL: row_mask for every row); NULL, NULL, 0xFFFFFFFF is the unfiltered call.  stack_max_out (or NULL):
 * the most stack entries any row held, never above rtxnp::stack_need().
 * rtxh_query_sweep_box_exhaustive: the same candidate functions over every sphere, plane and (instance, slot) without a node test, the same
 * order rule.  The walk's t is never below the exhaustive t, and where the two are equal the answers are identical.
 * rtxh_sweep_box_bound(S, W, T, kappa): rtxbs::sweep_box_bound, the bound in distance of ACCURACY in that header.
 * rtxh_sweep_box_triangle / _sphere / _plane: one candidate function at the row's world frame (an identity instance): 1 and t (axis) when
 * the primitive yields a candidate, else 0; bound is the walk's current t.
 * RTX_ERR_INVALID_ARG: five NULL outputs and the argument rules of rtxh_query_nearest; RTX_ERR_LIMIT: a tree deeper than RTX_MAX_STACK entries;
 * RTX_ERR_STATE: a non-rigid instance (the walk only), as for rtxh_query_nearest. */
int rtxh_query_sweep_box(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, float * t_out, float * normal_out, int32_t * object_id_out, int32_t * triangle_id_out,
                         int32_t * axis_out, int32_t * stack_max_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
int rtxh_query_sweep_box_exhaustive(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, float * t_out, float * normal_out, int32_t * object_id_out,
                                    int32_t * triangle_id_out, int32_t * axis_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
float rtxh_sweep_box_bound(float local_scale, float world_scale, float travelled, float kappa);
int rtxh_sweep_box_triangle(const float row[14], float bound, const rtx_triangle_hot * tri, float * t_out, int32_t * axis_out);
int rtxh_sweep_box_sphere(const float row[14], float bound, const rtx_sphere * sphere, float * t_out);
int rtxh_sweep_box_plane(const float row[14], const rtx_plane * plane, float * t_out);

/* The filtered walk queries (include/rtx.h: filtered queries) on the host: the same walks with FILTER's predicates of csrc/rtx_nearest_math.h,
 * so they give the device's bits.  The arguments of the function without the suffix, then object_masks (M = instance_count + sphere_count +
 * plane_count masks in the numbering of RTX_AOV_OBJECT_ID, or NULL: all ones), row_masks (n masks, or NULL: row_mask for every row) and
 * row_mask.  The _exhaustive_filtered forms search the visible primitives only: the promises of the three headers hold against them.
 * The functions without the suffix are unchanged: the same walk over a scene that hides nothing.  Errors as without the suffix.            */
int rtxh_query_nearest_filtered(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out, int32_t * stack_max_out,
                                const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
int rtxh_query_nearest_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                           const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
int rtxh_query_hits_filtered(const rtxh_nearest_scene * scene, const float * segments, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                             int32_t * count_out, int32_t * stack_max_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
int rtxh_query_hits_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * segments, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                                        int32_t * count_out, const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
int rtxh_query_sweep_filtered(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, uint32_t channels, const rtx_query_buffers * out, int32_t * stack_max_out,
                              const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
int rtxh_query_sweep_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * sweeps, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                         const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);

/* rtx_blas_pseudonormals (include/rtx.h) on the host, by the code the kernels run (csrc/rtx_side_math.h, whose header comment is the
 * specification: FACE, ANGLE, VERTEX, EDGE): the angle-weighted pseudonormal tables of an indexed mesh — positions V*3, indices T*3 (the SOURCE
 * topology; an index outside [0, V) makes a triangle invalid), slot_vertices slots*3 (the vertices of every triangle slot of the BLAS, -1 for a
 * pad slot), vert_out V*4, edge_out slots*3*4 (either may be NULL; w of every record is 0).  Written as the plain loop over triangles and
 * corners, where the device gathers through a sorted inverted index: the same additions in the same order, the same bits.  No output
 * component is NaN or infinite.  RTX_ERR_INVALID_ARG: a null pointer that is needed, T < 1, V < 1, slots < 0, nothing to write.            */
int rtxh_blas_pseudonormals(const float * positions, const int32_t * indices, int32_t triangle_count, int32_t vertex_count,
                            const int32_t * slot_vertices, int32_t slots, float * vert_out, float * edge_out);
/* rtx_query_signed_distance (include/rtx.h) on the host: rtxh_query_nearest (or its _exhaustive / _filtered forms), then SIDE of
 * csrc/rtx_side_math.h for every row's winner — the device's bits.  side: one rtxh_side_blas per BLAS id of the scene (tables as
 * rtxh_blas_pseudonormals or rtx_read_blas_pseudonormals give them; a null pointer in an entry: that mesh has no tables, feature + 8), or
 * NULL: no mesh has tables.  signed_out: n floats, required; feature_out: n codes or NULL.  channels may be 0, and then out may be NULL.
 * Errors otherwise as for the function it extends.                                                                                       */
typedef struct rtxh_side_blas { const float * vert_pn; const float * edge_pn; const int32_t * slot_vertices; int32_t vertex_count, pad; } rtxh_side_blas;
int rtxh_query_signed_distance(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                               const rtxh_side_blas * side, float * signed_out, int32_t * feature_out, int32_t * stack_max_out);
int rtxh_query_signed_distance_filtered(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                        const rtxh_side_blas * side, float * signed_out, int32_t * feature_out, int32_t * stack_max_out,
                                        const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);
int rtxh_query_signed_distance_exhaustive(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                          const rtxh_side_blas * side, float * signed_out, int32_t * feature_out);
int rtxh_query_signed_distance_exhaustive_filtered(const rtxh_nearest_scene * scene, const float * points, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                                   const rtxh_side_blas * side, float * signed_out, int32_t * feature_out,
                                                   const uint32_t * object_masks, const uint32_t * row_masks, uint32_t row_mask);

/* Texture::load (Texture.cpp:30-129): decodes a .png or .tga file the way the reference's vendored stb_image v2.19 does with
 * STBI_rgb_alpha (Texture.cpp:40), converts r,g,b bytes to linear light (colour_unpack :13-20, Math::gamma_to_linear Math.h:67-77;
 * alpha is dropped) and, when mipmap_mode != 0 (TEXTURE_SAMPLE_MODE_MIPMAP) and both sides are powers of two, appends the
 * box-filter chain.  *texels_out is malloc'ed (free with rtxh_texture_free) and holds *texel_count_out float3 texels, ready for
 * rtx_upload_texture.  Returns RTX_ERR_STATE if the file cannot be read, RTX_ERR_LIMIT for an image format stb_image knows
 * but this loader does not (JPEG, BMP, GIF, PSD, PIC, PNM, HDR), RTX_ERR_INVALID_ARG for a corrupt file (the reference aborts). */
int rtxh_texture_load(const char * path, int32_t mipmap_mode, float ** texels_out, int64_t * texel_count_out, rtx_texture_desc * desc);
int rtxh_texture_free(float * texels);
/* Sky::Sky (Sky.cpp:8-26): reads a square angular-map probe stored as raw float3 texels (`Data/Sky_Probes/<name>.float`); the result goes to
 * rtx_upload_sky.  *texels_out is malloc'ed (free with rtxh_texture_free).  A file whose texel count is not a square is refused.     */
int rtxh_sky_load(const char * path, float ** texels_out, int32_t * size_out);
/* The decode step alone: width*height RGBA8 pixels, top row first (malloc'ed; free with rtxh_image_free). */
int rtxh_image_load(const char * path, int32_t * width, int32_t * height, uint8_t ** rgba_out);
int rtxh_image_free(uint8_t * rgba);
/* Screenshot: a frame in Window::frame_buffer layout (0x00RRGGBB, e.g. from rtx_read_framebuffer or rtx_present) as an RGB PNG. */
int rtxh_image_save_png(const char * path, const uint32_t * packed, int32_t width, int32_t height);

/* Procedural "atrium": returns the triangle count for a detail level, then fills caller arrays.   */
typedef struct rtxh_mesh {
    float *   positions;     /* n*9  */
    float *   normals;       /* n*9  */
    float *   texcoords;     /* n*6  (already in the reference's convention: v flipped, OBJLoader.cpp:139-141) */
    int32_t * material_ids;  /* n    (mesh-local) */
    int32_t   triangle_count;
    int32_t   material_count;
} rtxh_mesh;
int rtxh_atrium_generate(uint32_t seed, int32_t detail, rtxh_mesh * out);   /* allocates; free with rtxh_mesh_free */
int rtxh_mesh_free(rtxh_mesh * m);

/* OBJ + MTL -> the triangle soup and material list OBJLoader::load_obj builds (OBJLoader.cpp:8-41,70-187).
 * materials[i].texture_id >= 0 means texture_names + i*RTXH_TEXNAME_MAX holds the map_Kd path (directory of the OBJ
 * prepended, as OBJLoader.cpp:21 does); decoding the image is left to the caller (Texture::load, Texture.cpp:30-129).   */
#define RTXH_TEXNAME_MAX 512
typedef struct rtxh_obj {
    rtxh_mesh      mesh;            /* material_ids are local to `materials` */
    rtx_material * materials;       /* mesh.material_count entries */
    char *         texture_names;   /* mesh.material_count * RTXH_TEXNAME_MAX bytes */
} rtxh_obj;
int rtxh_obj_load(const char * path, rtxh_obj * out);                        /* allocates; free with rtxh_obj_free */
int rtxh_obj_free(rtxh_obj * o);
/* OBJLoader::load_mtl (OBJLoader.cpp:43-68): materials only, from the .mtl named like the OBJ — what BottomLevelBVH::load registers when the
 * geometry comes from a `.bvh` cache file (BottomLevelBVH.cpp:28-33).  out->mesh stays empty except material_count.                          */
int rtxh_mtl_load(const char * obj_path, rtxh_obj * out);

/* `<mesh>.obj.bvh` cache files exactly as BottomLevelBVH::save_to_disk / load_from_disk read and write them (BottomLevelBVH.cpp:149-192).
 * The arrays are NOT flattened: triangle i of a leaf is hot[indices[i]] (BottomLevelBVH::flatten, :196-212, is the caller's gather).          */
typedef struct rtxh_bvh_cache {
    int32_t triangle_count, node_count, index_count, pad;
    rtx_triangle_hot *  hot;       /* triangle_count */
    rtx_triangle_cold * cold;      /* triangle_count */
    rtx_bvh_node *      nodes;     /* node_count */
    int32_t *           indices;   /* index_count */
} rtxh_bvh_cache;
int rtxh_bvh_cache_load(const char * path, rtxh_bvh_cache * out);            /* allocates; free with rtxh_bvh_cache_free */
int rtxh_bvh_cache_save(const char * path, const rtxh_bvh_cache * cache);
int rtxh_bvh_cache_free(rtxh_bvh_cache * cache);

#ifdef __cplusplus
}
#endif
#endif
