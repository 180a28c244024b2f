/*
 * rtx.h — C ABI of the MI355X (gfx950) render path.
 *
 * This is the drop-in boundary for the one hot path of clayne/CPU-Raytracer:
 *
 *   Raytracer::render_tile -> Raytracer::bounce -> Scene::trace_primitives /
 *   Scene::intersect_primitives -> TopLevelBVH / Mesh / BottomLevelBVH ->
 *   triangle / Sphere / Plane tests -> Light::calc_lighting -> recursive
 *   reflect / refract with ray differentials -> Texture::sample / Sky::sample
 *   -> Window::plot
 *
 * The reference has no FFI of its own; its seam is three C++ entry points
 * (reference file:line given with each function below).  Every function here
 * takes plain pointers and sizes only, returns an int status (RTX_OK == 0)
 * instead of the reference's printf + abort(), copies caller-owned host
 * buffers before returning, and is implemented by librtx_hip.so (hand-written
 * HIP for gfx950).  There is no CPU fallback behind this ABI: without a HIP
 * device rtx_create() fails with RTX_ERR_NO_DEVICE.
 *
 * Record layouts marked "reference layout" are byte-identical to the
 * reference's lane-1 structs so that its flattened BottomLevelBVH arrays and
 * its `.bvh` cache files (BottomLevelBVH.cpp:149-192) can be handed over
 * without conversion.
 */
#ifndef RTX_H
#define RTX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_ABI_VERSION 1

/* ---- status codes (the reference aborts; we return) -------------------- */
enum {
    RTX_OK               = 0,
    RTX_ERR_INVALID_ARG  = 1,  /* null pointer, negative count, bad id      */
    RTX_ERR_NO_DEVICE    = 2,  /* no HIP device / device ordinal not present */
    RTX_ERR_HIP          = 3,  /* a HIP runtime call failed (see rtx_last_error) */
    RTX_ERR_LIMIT        = 4,  /* MAX_MATERIALS (Config.h:18), stack size, texture count ... */
    RTX_ERR_STATE        = 5,  /* render before set_frame / missing BLAS ...  */
    RTX_ERR_OOM          = 6
};

/* ---- Config.h knobs (reference Config.h:1-55) --------------------------- */
enum { RTX_TRAVERSE_NAIVE = 0, RTX_TRAVERSE_ORDERED = 1 };            /* Config.h:27-30 */
enum { RTX_TEXTURE_NEAREST = 0, RTX_TEXTURE_BILINEAR = 1, RTX_TEXTURE_MIPMAP = 2 }; /* Config.h:38-42 */
enum { RTX_MIP_TRILINEAR = 0, RTX_MIP_ANISOTROPIC = 1, RTX_MIP_EWA = 2 };           /* Config.h:49-53 */

#define RTX_MAX_MATERIALS   256   /* Config.h:18  MAX_MATERIALS            */
#define RTX_MAX_STACK       64    /* Config.h:25  BVH_TRAVERSAL_STACK_SIZE */
#define RTX_MAX_MIP_LEVELS  16
#define RTX_TILE_SIZE       32    /* Window.h:32-33 tile_width/tile_height */
#define RTX_EWA_LUT_SIZE    128   /* Texture.h:53                          */

typedef struct rtx_config {
    int32_t width;               /* SCREEN_WIDTH                                    */
    int32_t height;              /* SCREEN_HEIGHT                                   */
    int32_t bounces;             /* NUMBER_OF_BOUNCES (0 = primary rays only)       */
    int32_t stack_size;          /* BVH_TRAVERSAL_STACK_SIZE, 1..RTX_MAX_STACK: a BVH with an inner node at depth d needs d + 2 entries of the
                                    reference's (unchecked) per-BVH stack; rtx_render_tiles refuses deeper trees with RTX_ERR_LIMIT */
    int32_t traversal_strategy;  /* BVH_TRAVERSAL_STRATEGY                          */
    int32_t texture_mode;        /* TEXTURE_SAMPLE_MODE                             */
    int32_t mip_filter;          /* MIPMAP_FILTER                                   */
    float   max_anisotropy;      /* MAX_ANISOTROPY                                  */
    int32_t device;              /* HIP device ordinal for this context             */
    int32_t heatmap;             /* BVH_VISUALIZE_HEATMAP (Config.h:23): pixels show BLAS traversal steps of the primary ray (Raytracer.cpp:97-102) */
    int32_t reserved[6];
} rtx_config;

/* ---- geometry records (reference layouts) ------------------------------ */
typedef struct rtx_bvh_node {          /* BVHNode.h:10-16, 32 B */
    float   aabb_min[3];
    float   aabb_max[3];
    int32_t left_or_first;             /* inner: index of left child (right = left+1); leaf: first primitive */
    int32_t count;                     /* bits 30-31: split axis (1=x,2=y,3=z); bits 0-29: leaf count (>0 = leaf) */
} rtx_bvh_node;

typedef struct rtx_triangle_hot {      /* BottomLevelBVH.h:6-10, 36 B */
    float position_0[3];
    float position_edge_1[3];
    float position_edge_2[3];
} rtx_triangle_hot;

typedef struct rtx_triangle_cold {     /* BottomLevelBVH.h:12-22, 64 B */
    float   tex_coord_0[2];
    float   tex_coord_edge_1[2];
    float   tex_coord_edge_2[2];
    float   normal_0[3];
    float   normal_edge_1[3];
    float   normal_edge_2[3];
    int32_t material_id;               /* OBJ-local id; global id = material_offset + this (BottomLevelBVH.cpp:265) */
} rtx_triangle_cold;

typedef struct rtx_material {          /* Material.h:7-14 (texture pointer replaced by a texture id) */
    float   diffuse[3];
    int32_t texture_id;                /* -1 = no texture */
    float   reflection[3];
    float   transmittance[3];
    float   index_of_refraction;
    int32_t pad;
} rtx_material;                        /* 48 B */

typedef struct rtx_texture_desc {      /* Texture.h:8-19 */
    int32_t width;
    int32_t height;
    int32_t mipmapped;                 /* Texture.cpp:49-55: both sides powers of two and mipmap mode */
    int32_t mip_levels;                /* 1 when not mipmapped */
    int32_t mip_offsets[RTX_MAX_MIP_LEVELS]; /* in texels, Texture.cpp:76-117 */
} rtx_texture_desc;

typedef struct rtx_instance {          /* Mesh.h:8-14 after Mesh::update (Mesh.cpp:9-15) */
    int32_t blas_id;
    int32_t pad[3];
    float   world[16];                 /* Transform::world_matrix, cells[i + 4*j] (Matrix4.h:19-23) */
    float   world_inv[16];             /* Mesh::transform_inv */
} rtx_instance;

typedef struct rtx_sphere {            /* Sphere.h:7-24 after Sphere::update */
    float   center[3];                 /* transform.position */
    float   radius_inv;
    float   radius_squared;
    int32_t material_id;               /* global material id (Primitive.h:6) */
} rtx_sphere;

typedef struct rtx_plane {             /* Plane.h:7-22 after Plane::update (Plane.cpp:3-11) */
    float   normal[3];                 /* world_normal */
    float   distance;                  /* world_distance */
    float   u_axis[3];
    float   v_axis[3];
    int32_t material_id;
    int32_t pad;
} rtx_plane;

typedef struct rtx_point_light {       /* PointLight.h:4-7 */
    float colour[3];
    float position[3];
} rtx_point_light;

typedef struct rtx_spot_light {        /* SpotLight.h:6-15 */
    float colour[3];
    float position[3];
    float negative_direction[3];
    float inner_cutoff;                /* cos(half inner angle) */
    float outer_cutoff;                /* cos(half outer angle) */
} rtx_spot_light;

typedef struct rtx_directional_light { /* DirectionalLight.h:4-7 */
    float colour[3];
    float negative_direction[3];
} rtx_directional_light;

typedef struct rtx_camera {            /* Camera.h:10-23 after Camera::update (Camera.cpp:44-47) */
    float position[3];
    float rotated_top_left_corner[3];
    float rotated_x_axis[3];
    float rotated_y_axis[3];
} rtx_camera;

/* Everything Scene::update (Scene.cpp:139-171) produces for one frame. */
typedef struct rtx_frame {
    rtx_camera camera;
    float      ambient[3];             /* Scene::ambient_lighting (Scene.h:33) */
    int32_t    pad0;

    const rtx_bvh_node * tlas_nodes;   /* TopLevelBVH::nodes (root = 0, index 1 unused) */
    int32_t              tlas_node_count;
    const int32_t *      tlas_indices; /* TopLevelBVH::indices: leaf slot -> instance */
    int32_t              tlas_index_count;
    const rtx_instance * instances;
    int32_t              instance_count;

    const rtx_sphere * spheres;                     int32_t sphere_count;
    const rtx_plane *  planes;                      int32_t plane_count;
    const rtx_point_light *       point_lights;       int32_t point_light_count;
    const rtx_spot_light *        spot_lights;        int32_t spot_light_count;
    const rtx_directional_light * directional_lights; int32_t directional_light_count;
} rtx_frame;

/* PerformanceStats (Raytracer.h:4-9), widened to 64 bit; counting rule of
 * Raytracer.cpp:61,163,180,192,265,320 at SIMD_LANE_SIZE == 1.            */
typedef struct rtx_stats {
    uint64_t num_primary_rays;
    uint64_t num_shadow_rays;
    uint64_t num_reflection_rays;
    uint64_t num_refraction_rays;
} rtx_stats;

/* Work counters behind the roofline accounting; filled by
 * rtx_render_tiles only when RTX_RENDER_COUNT_WORK is set (slower kernels). */
typedef struct rtx_work_counters {
    uint64_t closest_rays;             /* rays through trace_primitives          */
    uint64_t any_rays;                 /* rays through intersect_primitives      */
    uint64_t tlas_nodes_closest;       /* TLAS nodes popped (slab tests)         */
    uint64_t tlas_nodes_any;
    uint64_t blas_nodes_closest;       /* BLAS nodes popped (slab tests)         */
    uint64_t blas_nodes_any;
    uint64_t instances_closest;        /* Mesh::trace entered                    */
    uint64_t instances_any;            /* Mesh::intersect entered                */
    uint64_t tri_tests_closest;        /* triangle_trace calls                   */
    uint64_t tri_tests_any;            /* triangle_intersect calls               */
    uint64_t triangle_hits;            /* closest hit is a triangle (cold fetch) */
    uint64_t shaded_hits;              /* material fetches                       */
    uint64_t sky_lookups;
    uint64_t texel_fetches;
    uint64_t rays_spawned;             /* secondary rays written to a queue      */
    uint64_t reserved[5];
} rtx_work_counters;

typedef struct rtx_ctx rtx_ctx;

/* ---- lifetime ----------------------------------------------------------- */

/* One context per GPU.  Replaces: Window(SCREEN_WIDTH, SCREEN_HEIGHT) framebuffer
 * allocation (Window.cpp:42,76), Texture::init() EWA table (Texture.h:53-62,
 * Main.cpp:25), MaterialBuffer::init() (Material.h:52-60, Main.cpp:26) and
 * WorkerThreads::init (WorkerThread.cpp:72-114).                              */
int rtx_create(const rtx_config * config, rtx_ctx ** out_ctx);
int rtx_destroy(rtx_ctx * ctx);
const char * rtx_last_error(const rtx_ctx * ctx);
int rtx_abi_version(void);

/* ---- scene data that lives across frames -------------------------------- */
/* BLAS, materials, textures and the sky belong to the context, not to a
 * frame.  Any of the uploads and allocs below (and rtx_alloc_blas,
 * rtx_alloc_texture further down) may be called at any time, also after
 * rtx_set_frame and under ids the context has never seen: the call waits for
 * the work already queued on the context's stream — which keeps the state it
 * was queued with — and takes effect at the NEXT render or query call,
 * however large the context's tables have become and wherever they now lie.
 * rtx_set_frame is needed only for what it carries itself: instances, TLAS,
 * spheres, planes, lights and the camera.  What a call must not leave behind
 * is checked at the next render or query call, not at the upload: a material
 * table that no longer covers an id in use is RTX_ERR_STATE there.  A call
 * that fails (RTX_ERR_OOM, RTX_ERR_HIP) leaves the table it was to replace,
 * its count and the ids in it as they were.                                   */

/* A flattened BottomLevelBVH (BottomLevelBVH.h:5-34 after flatten(),
 * BottomLevelBVH.cpp:196-212): nodes, and hot/cold triangles already in leaf
 * order.  Replaces BottomLevelBVH::load (BottomLevelBVH.cpp:18-59).          */
int rtx_upload_blas(rtx_ctx * ctx, int32_t blas_id,
                    const rtx_bvh_node * nodes, int32_t node_count,
                    const rtx_triangle_hot * tri_hot, const rtx_triangle_cold * tri_cold,
                    int32_t triangle_count, int32_t material_offset);

/* The global MaterialBuffer::materials[] (Material.h:28-61); index 0 is the
 * all-zero default material.                                                 */
int rtx_upload_materials(rtx_ctx * ctx, const rtx_material * materials, int32_t count);

/* One Texture (Texture.h:8-19): linear-space float3 texels, mip chain
 * appended as Texture::load builds it (Texture.cpp:58-117).  Accepted: any
 * width, height >= 1 (sides that are no power of two wrap by modulo); 1 ..
 * RTX_MAX_MIP_LEVELS levels where level l is (width >> l) x (height >> l)
 * texels at mip_offsets[l], every level non-empty and inside texel_count
 * (so at most 1 + log2(min(width, height)) levels; non-square chains, one-
 * level "chains" and chains on a base that is no power of two included).
 * Anything else: RTX_ERR_INVALID_ARG, and the id keeps what it held.  An id
 * may be uploaded again with another shape.                                  */
int rtx_upload_texture(rtx_ctx * ctx, int32_t texture_id, const rtx_texture_desc * desc,
                       const float * texels_rgb, int64_t texel_count);

/* Sky (Sky.cpp:8-26): size*size float3 texels.                               */
int rtx_upload_sky(rtx_ctx * ctx, const float * texels_rgb, int32_t size);

/* ---- per frame ------------------------------------------------------------ */

/* The result of Scene::update(delta) (Scene.cpp:139-171): camera basis,
 * instance matrices, rebuilt TLAS, analytic primitives, lights.  Must be
 * called before rendering, never concurrently with it (Main.cpp:54-57).
 * The instances' world / world_inv are taken as given, 16 floats each: any
 * finite matrix is rendered and traced in the instance's local ray (rigid,
 * scaled, mirrored, sheared, singular).  A NaN or infinite cell is
 * RTX_ERR_INVALID_ARG and nothing changes: the previous frame stays bound.
 * Finite cells can still carry a far origin to a non-finite local origin
 * (|cell| * |origin| beyond FLT_MAX), which the packet kernels do not
 * survive: keep matrices and origins within what fp32 multiplies.  Whether
 * every instance is a rigid pose is decided here, for the length queries
 * (rtx_query_nearest: Limits).                                               */
int rtx_set_frame(rtx_ctx * ctx, const rtx_frame * frame);

enum {
    RTX_RENDER_COUNT_WORK = 1,         /* also fill rtx_work_counters (instrumented kernels) */
    RTX_RENDER_SIMPLE_TRACE = 2,       /* use the plain pop-and-test traversal kernels (A/B reference for the pair-fetch kernels) */
    RTX_RENDER_SERIAL = 8,             /* launch every kernel on ONE stream: closest-hit + shade per level, then a single shadow-ray
                                          launch for all levels, then resolve.  Use when several contexts render consecutive
                                          frames concurrently (one stream each); the default (two streams, shadow rays of level 0
                                          overlapping the deeper levels) gives the lowest latency for one frame at a time          */
    RTX_RENDER_LANE_TRACE = 16,        /* A/B: round 1's per-lane traversal kernels (persistent threads with lane refill, csrc/rtx_trace.h
                                          k_trace_fast) instead of the hybrid wave-packet kernels (csrc/rtx_packet.h).  Frames are bit-identical. */
    RTX_RENDER_PACKET_STATS = 32,      /* instrumented packet kernels: rtx_work_counters::reserved[0..4] = packets walked, child-pair steps,
                                          triangle steps, and the lane occupancy sums of both                                                 */
    RTX_RENDER_PACKET_CLOSEST = 64,    /* A/B: closest-hit packets walk the shared top of the tree together too (same threshold as shadow-ray packets);
                                          by default every lane of a closest-hit packet walks its own ray from the BLAS root (private stacks in
                                          LDS), which is faster until the shared part of that walk is hand-scheduled like the shadow-ray
                                          kernel's.  Frames are bit-identical either way.                                                   */
    RTX_RENDER_CULL_DEAD_SHADOW_RAYS = 4, /* count, but do not traverse, shadow rays whose unshadowed light contribution is exactly 0
                                          (N.L <= 0 or outside a spot cone): the pixel cannot depend on them.  Frames and
                                          rtx_stats are bit-identical with and without this flag.                                   */
    RTX_RENDER_AOV = 128               /* also write the channels bound by rtx_bind_aovs for every primary ray of the call (see below).
                                          Frames and rtx_stats are bit-identical with and without this flag.                        */
};

/* Renders tiles first_tile + i*tile_stride, i in [0, tile_count), numbered as
 * WorkerThread.cpp:57-61 (task -> x = (task % tile_count_x)*32, y = (task /
 * tile_count_x)*32, clipped at the right/bottom edge), each exactly as
 * Raytracer::render_tile (Raytracer.cpp:3-85) would, into the context's
 * device framebuffer.  Replaces wake_up_worker_threads + wait_on_worker_threads
 * (WorkerThread.cpp:116-129).  Returns after the work has been queued on the
 * context's stream; stats/work (may be NULL) are valid after rtx_synchronize
 * or any read-back call.                                                       */
int rtx_render_tiles(rtx_ctx * ctx, int32_t first_tile, int32_t tile_stride, int32_t tile_count,
                     uint32_t flags);
int rtx_synchronize(rtx_ctx * ctx);
int rtx_get_stats(rtx_ctx * ctx, rtx_stats * stats, rtx_work_counters * work);

/* Window::plot sink (Window.h:56-65).  rgb_f32: width*height*3 floats (linear,
 * before quantisation); packed_u32: width*height 0x00RRGGBB words.  Either
 * may be NULL.  Pixels of tiles that were never rendered are zero.            */
int rtx_read_framebuffer(rtx_ctx * ctx, float * rgb_f32, uint32_t * packed_u32);

/* Window::draw_quad (Window.cpp:87-95): what the window would show.  The packed frame is drawn through the reference's
 * full-screen shaders — gamma 1/2.2 and, with enable_fxaa (ENABLE_FXAA, Config.h:20), Data/Shaders/fragment_fxaa.glsl — by one
 * HIP kernel queued behind the frame.  display_u32 (host, width*height 0x00RRGGBB, may be NULL) receives the image after a
 * stream synchronise; *display_dev (may be NULL) its device address.  Parity with the GL path is UNPINNED (no GL driver to run
 * the reference's shaders); the kernel equals oracle `orc_present` bit for bit, which documents the conventions assumed.        */
int rtx_present(rtx_ctx * ctx, int32_t enable_fxaa, uint32_t * display_u32, void ** display_dev);

/* Device addresses of the same two buffers (for RCCL / zero-copy consumers). */
int rtx_framebuffer_device_ptrs(rtx_ctx * ctx, void ** rgb_f32_dev, void ** packed_u32_dev);

/* Render into caller-owned device buffers (e.g. tensors of a framework that also owns the RCCL
 * communicator) instead of the context's own framebuffer; NULL restores the internal one.  The
 * buffers must hold width*height*3 floats and width*height uint32.                                */
int rtx_bind_framebuffer(rtx_ctx * ctx, void * rgb_f32_dev, void * packed_u32_dev);

/* Enqueue all work of this context on a caller-owned HIP stream (hipStream_t passed as void *);
 * NULL restores the context's own stream.  Lets a caller order rendering against its own
 * kernels / collectives without host synchronisation.                                              */
int rtx_set_stream(rtx_ctx * ctx, void * hip_stream);

/* ---- several camera views of one frame ------------------------------------------------------------------------------------------
 * N views of the same scene state (stereo pairs, cube maps, a camera path, multi-view image sets) in ONE render call: the tiles of
 * all views are one batch of work, so a small frame fills the GPU and the launch floors of a call are shared by its views.  The
 * view framebuffer is separate from the context's framebuffer: rtx_render_tiles, rtx_read_framebuffer, rtx_present and the
 * rtx_group_* path behave as before and use the rtx_set_frame camera, whatever views are set.  Per-view scene state, resolution
 * or stats are not supported.                                                                                                     */
#define RTX_MAX_VIEWS 4096
/* Cameras of a batch of views of the current frame.  Everything else (TLAS, instances, primitives, lights, ambient) comes from the
 * last rtx_set_frame.  The cameras are copied before return, stream-ordered like rtx_set_frame: work already queued keeps the old ones.
 * RTX_ERR_INVALID_ARG: view_count < 1, > RTX_MAX_VIEWS, or view_count * width * height >= 2^31.                                    */
int rtx_set_views(rtx_ctx * ctx, const rtx_camera * cameras, int32_t view_count);
/* Render every tile of views [first_view, first_view + view_count).  Each view comes out exactly as rtx_render_tiles(ctx, 0, 1, all,
 * flags) would after rtx_set_frame with that view's camera.  View v goes to the view framebuffer at rgb[v*W*H*3 ...] and
 * packed[v*W*H ...].  rtx_get_stats afterwards = totals over the rendered views.  Every RTX_RENDER_* flag and the heat-map config
 * are honoured.  RTX_ERR_STATE before rtx_set_frame or rtx_set_views; RTX_ERR_INVALID_ARG for a range outside the views set or
 * outside a bound view framebuffer.  Queued like rtx_render_tiles.                                                                 */
int rtx_render_views(rtx_ctx * ctx, int32_t first_view, int32_t view_count, uint32_t flags);
/* views [first_view, first_view + view_count) of the view framebuffer (waits for the context's stream); either pointer may be NULL.
 * The range may reach as far as the views set or the ray views set or bound (rtx_set_rays / rtx_bind_rays), whichever are more.
 * Pixels of views that were never rendered are zero.                                                                              */
int rtx_read_views(rtx_ctx * ctx, int32_t first_view, int32_t view_count, float * rgb_f32, uint32_t * packed_u32);
/* Render views into caller-owned device buffers of view_capacity views (e.g. torch tensors [V,H,W,3] f32 / [V,H,W] i32) instead of
 * the context's own view framebuffer (allocated on first use, grown only); both NULL restores the own one.  Does not wait: work
 * already queued keeps writing the buffers it was queued with.                                                                     */
int rtx_bind_view_framebuffer(rtx_ctx * ctx, void * rgb_f32_dev, void * packed_u32_dev, int32_t view_capacity);

/* ---- ray views: caller-supplied primary rays ------------------------------------------------------------------------------------
 * V images of width x height primary rays that are not a rtx_camera's: fisheye, equirectangular or orthographic cameras, a lidar scan
 * pattern (64 x 1024 beams = a 1024 x 64 context), lens distortion, rolling shutter, a re-render of some pixels.  The layout is raster:
 * ray view*W*H + y*W + x belongs to the pixel with that index, the pixel index of the view framebuffer and of the AOVs.  Output goes
 * where rtx_render_views puts it: the view framebuffer (own, or rtx_bind_view_framebuffer; rtx_read_views) and, with RTX_RENDER_AOV,
 * the bound AOV channels at the view pixel index.
 * Pixel p gets exactly Raytracer::bounce(ray_p, NUMBER_OF_BOUNCES) with one defined change: `to_camera` (Raytracer.cpp:152) is at every
 * depth normalize(origin_p - hit.point), origin_p = the origin of the pixel's own primary ray (for the rays of a pinhole camera that is
 * the camera position: nothing changes).  Directions are used as given — the caller normalises them; distances are in units of
 * |direction|.  The differentials feed the texture LOD exactly like a camera ray's.
 * A ray whose direction is exactly (+-0, +-0, +-0) is no ray: its slot is treated like a clipped slot of an edge tile — nothing is
 * written to colour or AOVs, it is not counted in rtx_stats, it spawns nothing.  Any other float values, NaN and inf included, are legal
 * input.  A ray with a NaN or infinite origin or direction component hits nothing in the reference's arithmetic (every hit test ends in a
 * comparison with a NaN, a zero or an infinite distance): it is counted, and its pixel is Sky::sample of its direction.
 * A packet is still 64 consecutive slots = one 8x8 pixel block: incoherent rays are legal but cost what incoherent packets cost
 * (lay rays that travel together out in 8x8 blocks where the camera model allows it).
 * Out of scope: heat-map mode (RTX_ERR_STATE), the rtx_group_* path, per-view resolution.  rtx_set_views state and ray state are
 * independent of each other.                                                                                                          */
typedef struct rtx_ray {            /* 72 B = the 18 floats of rtx_debug_trace_rays */
    float origin[3], direction[3], dO_dx[3], dO_dy[3], dD_dx[3], dD_dy[3];
} rtx_ray;
/* view_count x height x width rays from host memory into the context's own ray buffer (grown only, freed by rtx_destroy).  Copied
 * before return and ordered on the context's stream like rtx_set_views: work already queued keeps the rays it was queued with.
 * RTX_ERR_INVALID_ARG: view_count < 1, > RTX_MAX_VIEWS, or view_count * width * height >= 2^31.                                       */
int rtx_set_rays(rtx_ctx * ctx, const rtx_ray * host_rays, int32_t view_count);
/* Rays in caller-owned device memory (e.g. a torch tensor [V,H,W,18] f32, 8-byte aligned) take the place of the own buffer; NULL
 * unbinds (the rays of rtx_set_rays, if any, are current again).  Does not wait: work already queued keeps the buffer it was queued
 * with, which must stay valid until that work is done.  The buffer is read when the work runs: values written into it (in stream
 * order) before a render call are the ones rendered.  Same RTX_ERR_INVALID_ARG cases as rtx_set_rays, and an address that is not 8-byte aligned.                                 */
int rtx_bind_rays(rtx_ctx * ctx, const void * rays_dev, int32_t view_count);
/* Render ray views [first_view, first_view + view_count) of the bound rays, else of the rays set.  Every RTX_RENDER_* flag is honoured.
 * rtx_get_stats afterwards = totals over the rendered ray views, num_primary_rays = the live rays.  RTX_ERR_STATE before rtx_set_frame,
 * before any rays are set or bound, or in heat-map mode; RTX_ERR_INVALID_ARG for view_count < 1 or > RTX_MAX_VIEWS, a range outside
 * the rays, outside a bound view framebuffer or (RTX_RENDER_AOV) outside the AOV capacity.  Queued like rtx_render_tiles.              */
int rtx_render_rays(rtx_ctx * ctx, int32_t first_view, int32_t view_count, uint32_t flags);

/* ---- per-pixel primary-hit AOVs (G-buffer channels) ---------------------------------------------------------------------------------
 * What Raytracer::bounce (Raytracer.cpp:87-145) knows about the PRIMARY ray of each pixel, written next to the colour by a render call
 * with RTX_RENDER_AOV.  The values are the frame's own: stored by the shading pass where it has them, not evaluated a second time.
 * Channel (bit)          per pixel    hit                                                        miss
 *   DEPTH                f32          RayHit::distance (RayHit.h:6), bounce's `distance` (:113)  +INFINITY (:107)
 *   POSITION             3 x f32      RayHit::point, world space (RayHit.h:8)                     0
 *   NORMAL               3 x f32      RayHit::normal, as shading uses it (RayHit.h:9)             0
 *   ALBEDO               3 x f32      Material::get_albedo: diffuse x Texture::sample with the    Sky::sample of the ray direction (:106)
 *                                     shading's LOD inputs (Material.h:16-22)
 *   UV                   2 x f32      RayHit::u, v (RayHit.h:12)                                  0
 *   MATERIAL_ID          i32          RayHit::material_id, global (RayHit.h:11)                   -1
 *   OBJECT_ID            i32          mesh instance i -> i (rtx_frame.instances); sphere s ->     -1
 *                                     instance_count + s; plane p -> instance_count + sphere_count + p
 *   TRIANGLE_ID          i32          index into the triangle arrays given to rtx_upload_blas     -1 (also for spheres and planes)
 *                                     for the instance's BLAS (flattened order, BottomLevelBVH.cpp:196-212)
 * Pixel index: y * width + x of a rtx_render_tiles call, view * width * height + y * width + x of a rtx_render_views call; only the
 * rendered pixels are written (clipped slots of edge tiles and tiles outside the call are left as they are).  Not available in
 * heat-map mode, nor on the rtx_group_* path.                                                                                        */
enum {
    RTX_AOV_DEPTH = 1, RTX_AOV_POSITION = 2, RTX_AOV_NORMAL = 4, RTX_AOV_ALBEDO = 8, RTX_AOV_UV = 16,
    RTX_AOV_MATERIAL_ID = 32, RTX_AOV_OBJECT_ID = 64, RTX_AOV_TRIANGLE_ID = 128,
    RTX_AOV_ALL = 255
};
typedef struct rtx_aov_buffers {       /* one pointer per channel, NULL = not written / not read */
    float   * depth;                   /* [pixels]     */
    float   * position;                /* [pixels][3]  */
    float   * normal;                  /* [pixels][3]  */
    float   * albedo;                  /* [pixels][3]  */
    float   * uv;                      /* [pixels][2]  */
    int32_t * material_id;             /* [pixels]     */
    int32_t * object_id;               /* [pixels]     */
    int32_t * triangle_id;             /* [pixels]     */
} rtx_aov_buffers;
/* Bind the channels in `channels` (RTX_AOV_* bits) for render calls with RTX_RENDER_AOV.  device != NULL: caller-owned device buffers of
 * pixel_capacity pixels each; a channel is written only if its bit is set and its pointer is not NULL.  device == NULL: the context's own
 * buffers (allocated on first use, grown only, like the view framebuffer; read with rtx_read_aovs).  channels == 0 unbinds.  Does not
 * wait: work already queued keeps writing the buffers it was queued with.  RTX_ERR_INVALID_ARG: unknown bits, or device != NULL with
 * pixel_capacity < 1.
 * A render call with RTX_RENDER_AOV returns RTX_ERR_STATE when nothing is bound or the context is in heat-map mode (no shading), and
 * RTX_ERR_INVALID_ARG when its pixel range — [0, width*height) for rtx_render_tiles, [0, (first_view + view_count)*width*height) for
 * rtx_render_views — exceeds pixel_capacity.  rtx_group_render* with it returns RTX_ERR_INVALID_ARG.                                 */
int rtx_bind_aovs(rtx_ctx * ctx, uint32_t channels, const rtx_aov_buffers * device, int64_t pixel_capacity);
/* pixels [first_view*W*H, (first_view + view_count)*W*H) of the context's own AOV buffers to host (waits for the context's stream); a
 * tiles call is (0, 1).  NULL host pointers are skipped.  RTX_ERR_STATE while caller buffers are bound; RTX_ERR_INVALID_ARG for a channel
 * whose own buffer does not hold the range (never bound, or bound for fewer pixels than rendered).                                  */
int rtx_read_aovs(rtx_ctx * ctx, int32_t first_view, int32_t view_count, const rtx_aov_buffers * host);

/* ---- device-side scene update -----------------------------------------------------------------------------------------------------------
 * The tail of Scene::update (Scene.cpp:166-170: Mesh::update for every instance, then the TLAS rebuild) on the device, for callers whose
 * object poses already live there (a simulation step, a learning loop): no copy to the host, no wait.
 * Poses of the instances of the current frame, from DEVICE memory: positions n x 3 f32, rotations n x 4 f32 (quaternion x, y, z, w —
 * Transform::position / rotation; any 4-byte aligned address).  Recomputes every rtx_instance (Mesh::update, Mesh.cpp:9-15: bit-identical to
 * rtxh_instance_update's records), the instances' world AABBs (AABB::transform, AABB.cpp:55-73) and a TLAS over them, on the context's
 * stream (rtx_set_stream: the caller's).  The TLAS is this project's own balanced tree, not the reference's SAH tree: rtxh_tlas_build_balanced
 * (include/rtx_host.h) documents it and builds the same bytes on the host.  blas_id of each instance, camera, ambient, spheres, planes and
 * lights stay as the last rtx_set_frame left them.  Does not wait for the device and reads nothing back: work already queued keeps the
 * state it was queued with, the next render call (any entry point, any flag) renders the updated scene; a later rtx_set_frame replaces the
 * state again.  The pose buffers are read when the work runs and must stay valid until then.
 * Any float values are legal poses, NaN and infinities included: such an instance may become invisible, the tree stays valid.
 * Checked in this order, the first that applies is returned and nothing changes: RTX_ERR_INVALID_ARG for a null or misaligned pointer or
 * instance_count < 1; RTX_ERR_LIMIT above RTX_UPDATE_MAX_INSTANCES; RTX_ERR_STATE before rtx_set_frame; RTX_ERR_INVALID_ARG for an
 * instance_count that is not the frame's; RTX_ERR_LIMIT when the tree of that many instances (deepest inner node at depth
 * ceil(log2 n) - 1) needs more than rtx_config.stack_size entries — the rule rtx_render_tiles applies to every BVH.  Heat-map contexts are supported.  Out of scope: the rtx_group_* path (every rank would
 * have to make the same call), world matrices or scale as input, spheres / planes / lights from device memory.  Vertices that move: rtx_refit_blas below. */
#define RTX_UPDATE_MAX_INSTANCES 65536
int rtx_update_instances(rtx_ctx * ctx, const void * positions_dev, const void * rotations_dev, int32_t instance_count);
/* The frame state the kernels currently read, to host (waits for the stream): rtx_instance records (instance_count of the frame), TLAS
 * nodes in the reference layout (rtx_bvh_node, root 0, index 1 unused; *tlas_node_count entries — call once with NULL arrays to learn the
 * count), TLAS indices (instance_count entries).  Any pointer may be NULL.  Handing the three arrays to rtx_set_frame of another context
 * gives that context the same frame.  RTX_ERR_STATE before rtx_set_frame.                                                                 */
int rtx_read_frame_state(rtx_ctx * ctx, rtx_instance * instances, rtx_bvh_node * tlas_nodes, int32_t * tlas_node_count,
                         int32_t * tlas_indices);

/* ---- device-side mesh refit ---------------------------------------------------------------------------------------------------------------
 * A mesh whose vertices move (cloth, a soft body, a skinned character, a learned deformation) with the positions in DEVICE memory: the BLAS
 * keeps its topology, its triangles and boxes are rewritten in place on the context's stream.  refit -> rtx_update_instances (which takes each
 * instance's root box from the device) -> render is a complete device-only frame update; the host copies nothing and waits for nothing.
 *
 * rtx_bind_blas_vertices, once per mesh, from HOST memory: slot_vertices[3k + c] = index of vertex c of the triangle in flattened slot k of the
 * arrays given to rtx_upload_blas (slot k = order_out[k] of any rtxh_blas_build*; the duplicated references of an SBVH repeat indices), every
 * index in [0, vertex_count).  May allocate and wait.  Uploads the table and a refit plan made from the uploaded topology (parents and arrival
 * counters for the bottom-up pass; for every slot of the 4-wide records the node whose box it carries, in the slot order chosen at upload),
 * and moves the mesh's box-plane lists into buffers of a fixed 2 * node_count floats per axis (duplicates allowed, padded with +inf: the
 * search only decides which walker a ray takes, never a result).  A mesh that kept the binary walk at upload keeps it.  Binding again replaces
 * the table; uploading the id again drops the binding.  RTX_ERR_INVALID_ARG: null pointer, bad id, vertex_count < 1, an index outside the
 * range; RTX_ERR_STATE: no BLAS uploaded under that id.
 *
 * rtx_refit_blas, per step, from DEVICE memory: positions vertex_count x 3 f32, normals vertex_count x 3 f32 or NULL (any 4-byte aligned
 * address).  Queued on the context's stream (rtx_set_stream: the caller's); never waits, allocates or reads back.  The buffers are read when
 * the work runs.  Rewrites every hot triangle (p0, p1 - p0, p2 - p0 in fp32); with normals the three normal fields of every cold triangle
 * (texture coordinates and material ids stay; NULL: the normals stay); the box of every node reachable from the root in all four device
 * layouts; the three sorted plane lists.  left_or_first, count, axis bits, the meta words of the wide records and unreachable node slots are
 * not touched, and whether the mesh takes the 4-wide walks is not decided again.  Boxes: a triangle's is AABB::from_points over its vertices,
 * then fix_if_needed (Triangle.h:17-22, AABB.h:26-32); a leaf's the union of its triangles' boxes in slot order, then fix_if_needed; an inner
 * node's the union of its children's STORED boxes, left first, then fix_if_needed (BVHPartitions.h:11-23).  rtxh_blas_refit (rtx_host.h)
 * builds the same bytes on the host from the same code.  Any float is a legal coordinate: a NaN or infinite component takes no part in a
 * box, so every reachable box stays finite with min <= max and nested in its parent; a triangle with such a vertex may become invisible, a
 * neighbour never.  A frame queued before the call renders the old mesh, the next render call (any entry point, any flag) the new one;
 * RTX_GRAPH=1 graphs stay valid (no pointer changes after the bind).  The instances' world boxes and the TLAS are NOT updated by this call:
 * follow with rtx_update_instances or rtx_set_frame when the root box moved.  Checked in this order, nothing changes on an error:
 * RTX_ERR_INVALID_ARG for a null or misaligned positions_dev or a misaligned normals_dev; RTX_ERR_STATE for an id that is not uploaded or
 * not bound; RTX_ERR_INVALID_ARG for a vertex_count that is not the bound one.  Normals of the moved vertices: rtx_blas_vertex_normals below; a
 * new topology: rtx_build_blas below.  Out of scope: the rtx_group_* path (every rank would have to make the same call).
 *
 * rtx_read_blas: what the kernels read now, to host (waits for the stream): node_count nodes in the reference layout, triangle_count hot and
 * cold records as given to rtx_upload_blas.  Any pointer may be NULL.  RTX_ERR_STATE: no BLAS uploaded under that id.                       */
int rtx_bind_blas_vertices(rtx_ctx * ctx, int32_t blas_id, const int32_t * slot_vertices, int32_t vertex_count);
int rtx_refit_blas(rtx_ctx * ctx, int32_t blas_id, const void * positions_dev, const void * normals_dev, int32_t vertex_count);
int rtx_read_blas(rtx_ctx * ctx, int32_t blas_id, rtx_bvh_node * nodes, rtx_triangle_hot * tri_hot, rtx_triangle_cold * tri_cold);

/* ---- device-side mesh build ---------------------------------------------------------------------------------------------------------------
 * A mesh whose tree no longer fits it (a deformation that tears neighbourhoods apart) or that did not exist a step ago (iso-surface extraction,
 * particles turned into triangles, a learned mesh), with the triangles in DEVICE memory: the BLAS is rebuilt on the context's stream.
 * build -> rtx_update_instances -> render is a complete device-only frame update; rebuild every N steps, rtx_refit_blas in between.
 *
 * rtx_alloc_blas, once per mesh, from HOST memory; may allocate and wait.  Creates under blas_id (replacing what the id held, like
 * rtx_upload_blas) a BLAS for up to triangle_count triangles over vertex_count vertices.  Its tree is this project's own balanced one, not the
 * reference's: rtxh_blas_build_balanced (include/rtx_host.h) documents it and builds the same bytes on the host.  The topology — an implicit heap
 * with leaves of at most 4 triangles — is a function of triangle_count alone, so everything the host decides from a BLAS before a launch (the
 * stack rules, whether the mesh takes the 4-wide walks and their stack needs, the slot order of the 4-wide records: smallest stack need first)
 * is decided here, as rtx_upload_blas would for that tree, and never again.  Uploads the four node layouts with their topology words, the
 * refit plan of rtx_bind_blas_vertices, zeroed triangle arrays, and allocates every scratch buffer of a build (keys, sort storage, plane lists
 * of 2 * node_count floats per axis).  material_ids: one OBJ-local id per SOURCE triangle, each >= 0, or NULL for all 0; a build carries them
 * to the slots.  Until the first build every triangle is invalid: the mesh is empty and legal to render.  Checked in this order, nothing changes
 * on an error: RTX_ERR_INVALID_ARG for a bad id, triangle_count < 1, vertex_count < 1 or a negative material id; RTX_ERR_LIMIT for
 * triangle_count >= 2^24 (the 4-wide walks' limit); RTX_ERR_LIMIT when the tree's deepest inner node (depth L - 1, L the first level with
 * ceil(triangle_count / 2^L) <= 4) needs more than rtx_config.stack_size entries — the rule rtx_update_instances applies.
 *
 * rtx_build_blas, per step, from DEVICE memory (any 4-byte aligned addresses): positions vertex_count x 3 f32, indices triangle_count x 3 i32,
 * normals vertex_count x 3 f32, texture coordinates vertex_count x 2 f32 or NULL (zeros), order_out triangle_count i32 or NULL: receives the
 * source triangle stored in each flattened slot, which is what RTX_AOV_TRIANGLE_ID reports.  Queued on the context's stream (rtx_set_stream: the
 * caller's); never waits, allocates or reads back.  The buffers are read when the work runs.  Every index is checked on the device against
 * [0, vertex_count): a triangle with any index outside is INVALID (-1 is the documented way to pad a mesh of fewer triangles) — nothing is read
 * through its indices, its hot record is nine quiet NaNs (0x7fc00000, stored), it takes no part in any box, sorts first, and stays invalid
 * through later refits whatever the positions.  Any float is a legal coordinate, as for the refit: every reachable box is finite with
 * min <= max and nested in its parent; a triangle with a non-finite vertex may become invisible, a neighbour never.  Rewrites all hot and cold
 * triangles, the slot table of the refit, the box of every node in all four layouts, the axis bits of `count` (both binary layouts) and of the
 * closest-hit 4-wide records' meta words, and the plane lists.  No pointer changes after the alloc: a frame queued before the call renders
 * the old mesh, the next render call (any entry point, any flag) the new one, RTX_GRAPH=1 graphs stay valid.  The TLAS is NOT updated: follow
 * with rtx_update_instances or rtx_set_frame.  Afterwards the mesh counts as bound for rtx_refit_blas(blas_id, positions, normals,
 * vertex_count), which keeps the topology and axis bits of the last build (the cold record of an invalid triangle stays as the build left it).
 * Checked in this order: RTX_ERR_INVALID_ARG for a null or misaligned positions / indices / normals pointer or a misaligned optional one;
 * RTX_ERR_STATE for an id that was not created by rtx_alloc_blas (or was uploaded again since).  Normals from positions: rtx_blas_vertex_normals
 * below.  Out of scope: per-triangle material ids from device memory, a SAH-quality device builder, the rtx_group_* path.                  */
int rtx_alloc_blas(rtx_ctx * ctx, int32_t blas_id, int32_t triangle_count, int32_t vertex_count, const int32_t * material_ids_host, int32_t material_offset);
int rtx_build_blas(rtx_ctx * ctx, int32_t blas_id, const void * positions_dev, const void * indices_dev, const void * normals_dev,
                   const void * texcoords_dev, void * order_out_dev);

/* ---- device-side vertex normals -------------------------------------------------------------------------------------------------------------
 * A caller with positions and an index buffer in DEVICE memory and no normals (cloth, a skinned character, a learned deformation, an extracted
 * iso-surface): smooth, area-weighted vertex normals computed on the context's stream into a device buffer that rtx_refit_blas and
 * rtx_build_blas take as it is.  normals -> refit (or build) -> rtx_update_instances -> render is a complete device-only step.  The result is
 * bit-reproducible — no float atomics: face vectors are stored, then summed per vertex in a fixed order — and bit-identical to
 * rtxh_vertex_normals (rtx_host.h), which runs the same arithmetic (csrc/rtx_normals_math.h) as a plain loop over triangles and corners.
 *   valid     a triangle is valid when its three indices lie in [0, vertex_count) (rtx_build_blas's rule; -1 pads a mesh).  Nothing is read
 *             through the indices of an invalid triangle, and it contributes to no vertex.
 *   face      e1 = p1 - p0, e2 = p2 - p0, f = e1 x e2 in unfused fp32: its length is twice the area, so the weighting is by area.  A face
 *             vector with a NaN or infinite component counts as (+0, +0, +0): a bad vertex spoils its own normal and never a neighbour's.
 *   sum       from (+0, +0, +0), f added once for every corner c = 3 * t + k that holds the vertex, in ascending c (a triangle that names a
 *             vertex twice adds its — zero — face vector twice).
 *   normal    m = max(|x|, |y|, |z|) of the sum.  m zero or not finite (a component of the sum is NaN or infinite): (+0, +0, +0).  Otherwise
 *             a = s / m, d = a.x * a.x + (a.y * a.y + a.z * a.z), normal = a / sqrtf(d), with correctly rounded '/' and sqrtf: unit length to
 *             2^-22 at any scale.  A vertex no valid triangle uses and a vertex whose contributions cancel get (+0, +0, +0): there is no
 *             tie rule beyond that.  No output component is ever NaN or infinite.
 *
 * rtx_alloc_blas_topology, once per mesh; may allocate and wait.  Allocates under blas_id everything the other two calls need for
 * triangle_count triangles over vertex_count vertices: the library's own copy of the indices, unsorted and sorted corner keys (3 *
 * triangle_count x 8 bytes each), the sort's temporary storage, vertex_count + 1 list offsets and one 16-byte face vector per triangle.  The
 * counts need not be the BLAS's own: an SBVH's slot table repeats triangles and would weight them twice, so the topology is the SOURCE index
 * buffer.  Calling it again replaces the state; rtx_upload_blas or rtx_alloc_blas over the id drops it.  Checked in this order, nothing
 * changes on an error: RTX_ERR_INVALID_ARG for a bad id, triangle_count < 1 or vertex_count < 1; RTX_ERR_LIMIT for triangle_count > 2^28
 * (corner indices and the sort's count are 32-bit); RTX_ERR_STATE when no BLAS is uploaded or allocated under the id.
 *
 * rtx_set_blas_topology, per topology (once for a refitted mesh, every step for a rebuilt one), from DEVICE memory: indices triangle_count x 3
 * i32 at any 4-byte aligned address, read when the work runs.  Queued on the context's stream (rtx_set_stream: the caller's); never waits,
 * allocates or reads back.  Copies the indices and builds the inverted index: the key of corner c is (uint64)v << 32 | c, v the vertex at that
 * corner, v = vertex_count for a corner of an invalid triangle (it sorts last); the keys are sorted (a total order: one result) and offset[v],
 * v in [0, vertex_count], is the lower bound of v << 32 among them.  RTX_ERR_INVALID_ARG for a null or misaligned pointer; RTX_ERR_STATE for an
 * id without rtx_alloc_blas_topology.
 *
 * rtx_blas_vertex_normals, per step, from DEVICE memory: positions vertex_count x 3 f32 in, normals_out vertex_count x 3 f32 out, caller-owned,
 * any 4-byte aligned addresses; exactly vertex_count x 12 bytes are written.  Queued like rtx_set_blas_topology; the buffers are read and
 * written when the work runs, in stream order with a following rtx_refit_blas / rtx_build_blas that reads normals_out.  Any float is a legal
 * coordinate.  A vertex of high valence (the pole of a UV sphere, the apex of a fan) is summed by one lane: splitting its list would change
 * the order of the additions and so the bits.  Checked in this order, nothing is queued on an error: RTX_ERR_INVALID_ARG for a null or
 * misaligned pointer; RTX_ERR_STATE for an id without an allocated topology; RTX_ERR_STATE when no rtx_set_blas_topology has been queued since
 * the alloc.  Out of scope: angle-weighted or crease-angle normals, flat normals, normals written straight into the cold records, the
 * rtx_group_* path, texture-space tangents.                                                                                               */
int rtx_alloc_blas_topology(rtx_ctx * ctx, int32_t blas_id, int32_t triangle_count, int32_t vertex_count);
int rtx_set_blas_topology(rtx_ctx * ctx, int32_t blas_id, const void * indices_dev);
int rtx_blas_vertex_normals(rtx_ctx * ctx, int32_t blas_id, const void * positions_dev, void * normals_out_dev);

/* ---- pseudonormal tables: the sign of a distance -----------------------------------------------------------------------------------------
 * What rtx_query_signed_distance (below) needs of a mesh to tell the two sides of its surface apart near edges and vertices, where the face
 * normal of the nearest triangle is wrong: the angle-weighted pseudonormals of Baerentzen and Aanaes (2005) — per vertex the sum of the unit
 * normals of its faces weighted by their corner angles, per edge the sum of the unit normals of the faces at the edge.  Computed on the
 * context's stream from positions in DEVICE memory, over the topology of rtx_set_blas_topology (the SOURCE index buffer) and the slot ->
 * vertex table of rtx_bind_blas_vertices / rtx_alloc_blas + rtx_build_blas.  Bit-reproducible — no float atomics: per-triangle records are
 * stored, then summed per vertex and per slot edge in ascending corner order — and bit-identical to rtxh_blas_pseudonormals (rtx_host.h).
 * The arithmetic (FACE, ANGLE, VERTEX, EDGE) is specified in the header comment of csrc/rtx_side_math.h.
 *
 * rtx_blas_pseudonormals, per step, after the positions of the mesh changed (r.refit_blas, then this): positions vertex_count x 3 f32 at any
 * 4-byte aligned address, read when the work runs.  The first call for an id allocates the tables (64 bytes per source triangle, 16 per
 * vertex, 48 per triangle slot) and may wait for the stream; a refused allocation changes nothing.  Later calls only queue three kernels, read
 * nothing back and move no pointer.  The tables are as current as the last call: a refit or a build without it leaves them stale (and, after
 * a build, indexed by the slots of the previous build) — the contract the vertex normals have.  rtx_upload_blas or rtx_alloc_blas over the
 * id, and rtx_alloc_blas_topology over the id, drop the tables: the mesh then has none (feature + 8) until the next call.  Checked in this
 * order, nothing is queued on an error: RTX_ERR_INVALID_ARG for a null ctx, a null or misaligned pointer; RTX_ERR_STATE for an id without an
 * allocated topology; RTX_ERR_STATE when no rtx_set_blas_topology has been queued since the alloc; RTX_ERR_STATE when no vertices are bound to
 * the id; RTX_ERR_INVALID_ARG when the topology's vertex_count is not the bound one; then RTX_ERR_OOM / RTX_ERR_HIP of the first call's
 * allocation.
 *
 * rtx_read_blas_pseudonormals (waits for the stream): vert_out vertex_count x 4 floats, edge_out slots x 3 x 4 floats (edge ab, bc, ac of
 * every triangle slot; w of every record is 0); either may be NULL.  RTX_ERR_INVALID_ARG for a null ctx, a bad id or two null outputs;
 * RTX_ERR_STATE for an id without tables.                                                                                              */
int rtx_blas_pseudonormals(rtx_ctx * ctx, int32_t blas_id, const void * positions_dev /* [V][3] f32 */);
int rtx_read_blas_pseudonormals(rtx_ctx * ctx, int32_t blas_id, float * vert_out /* [V][4] */, float * edge_out /* [slots][3][4] */);

/* ---- device-side texture and sky update -----------------------------------------------------------------------------------------------
 * What the surfaces look like, with the texels in DEVICE memory: a render shown on a screen or a portal inside the scene (a view
 * framebuffer is [h][w][3] f32 in linear light), a decoded video frame, a generated albedo, an animated environment probe.  update -> render
 * is a complete device-only step: the host copies nothing, filters nothing and waits for nothing.
 *
 * rtx_alloc_texture, once per texture, from the host; may allocate and wait.  Creates under texture_id (replacing what the id held, exactly as
 * rtx_upload_texture does, its wait before an old texel array is released included) a texture of width x height with the shape Texture::load
 * gives it (Texture.cpp:49-55, 76-117): with mipmapped != 0 and both sides powers of two, mip_levels = 1 + (int)log2f(min(width, height))
 * levels, level l (width >> l) x (height >> l) texels at the cumulative offset from width * height; otherwise one level (mipmapped = 0 in
 * the descriptor).  The whole chain is allocated and zeroed: a texture that was never updated is black and legal to render.  Uploads the
 * texture table and, once per context, the 256-entry byte -> linear table of RTX_TEXELS_RGBA8_SRGB, computed on the host with the expression
 * and the libm of rtxh_texture_load: the device never evaluates powf.  Checked in this order, nothing changes on an error:
 * RTX_ERR_INVALID_ARG for an id outside [0, 4096), width < 1 or height < 1; RTX_ERR_LIMIT for a chain of more than RTX_MAX_MIP_LEVELS
 * levels or of more texels than the int32_t offsets of rtx_texture_desc hold.
 *
 * rtx_update_texture, per step, from DEVICE memory: width x height texels of `format` (any address aligned to the element: 4 bytes for
 * RTX_TEXELS_RGB_F32, 1 for RTX_TEXELS_RGBA8_SRGB).  Queued on the context's stream (rtx_set_stream: the caller's); never waits, allocates
 * or reads back.  The buffer is read when the work runs.  Rewrites level 0 and every further level of the chain: a level is computed from
 * the STORED fp32 texels of the level before it, (((c0 + c1) + c2) + c3) * 0.25f per channel with c0 = (2i, 2j), c1 = (2i + 1, 2j),
 * c2 = (2i, 2j + 1), c3 = (2i + 1, 2j + 1) (Texture.cpp:99-104) — rtxh_texture_mips (rtx_host.h) builds the same bits on the host from the
 * same code.  Any float is a legal texel (NaN, infinities, subnormals: nothing is flushed or clamped; which NaN a sum such as inf + -inf
 * yields is the machine's).  No pointer and no descriptor field changes: a frame queued before the call samples the old texels, the next
 * render call (any entry point, any flag) the new ones, RTX_GRAPH=1 graphs stay valid.  Checked in this order: RTX_ERR_INVALID_ARG for a null
 * or misaligned texels_dev or an unknown format; RTX_ERR_STATE for an id that was not created by rtx_alloc_texture (or was uploaded again
 * with rtx_upload_texture since).
 *
 * rtx_read_texture: what the samplers read now, of any uploaded or allocated id, to the host (waits for the stream; plain copies, nothing
 * is launched and nothing changes, like rtx_read_blas).  *desc receives the descriptor, texels_rgb the chain as float3 in the layout
 * rtx_upload_texture takes, from texel 0 to the end of the level that ends last: the largest mip_offsets[l] + (width >> l) * (height >> l)
 * over the levels, which is every texel a sampler can read (for a chain laid out in level order, the end of the last level; texels a
 * caller uploaded behind that end belong to no level and are not returned).  Either pointer may be NULL: call once with texels_rgb NULL
 * to learn the size from the descriptor.  RTX_ERR_INVALID_ARG for a bad id, or a
 * capacity_texels too small for a non-NULL texels_rgb; RTX_ERR_STATE for an id that holds nothing.
 *
 * rtx_update_sky: size x size float3 texels from DEVICE memory (4-byte aligned) over the probe rtx_upload_sky made: ONE copy on the
 * context's stream, device to device; never waits or allocates.  The padding texel behind the probe (Sky.cpp:45's inclusive clamp) stays
 * zero, the pointer and the size stay.  A frame queued before the call shows the old sky.  RTX_ERR_INVALID_ARG for a null or misaligned
 * pointer; RTX_ERR_STATE before rtx_upload_sky; RTX_ERR_INVALID_ARG for a size that is not the uploaded one.
 *
 * Out of scope: materials from device memory (their texture ids are validated on the host before a launch; a device-side table would need
 * a device-side check); updating a texture made by rtx_upload_texture (its chain may be the caller's own); formats other than the two
 * below; per-view textures; the rtx_group_* path (every rank would have to make the same call); another size without a new alloc.        */
enum { RTX_TEXELS_RGB_F32 = 0,      /* [h][w][3] float, linear light: what rtx_upload_texture takes as level 0, what a view framebuffer holds */
       RTX_TEXELS_RGBA8_SRGB = 1 }; /* [h][w][4] uint8 r,g,b,a as stbi_load(..., STBI_rgb_alpha) returns them: colour_unpack + Math::gamma_to_linear per byte, alpha dropped */
int rtx_alloc_texture (rtx_ctx * ctx, int32_t texture_id, int32_t width, int32_t height, int32_t mipmapped);
int rtx_update_texture(rtx_ctx * ctx, int32_t texture_id, const void * texels_dev, int32_t format);
int rtx_read_texture  (rtx_ctx * ctx, int32_t texture_id, rtx_texture_desc * desc, float * texels_rgb, int64_t capacity_texels);
int rtx_update_sky    (rtx_ctx * ctx, const void * texels_dev, int32_t size);

/* ---- ray queries -----------------------------------------------------------------------------------------------------------------------
 * Questions to the scene without rendering a frame: n arbitrary rays -> the closest hit of each, n segments -> whether each is blocked.
 * For sensors with non-rectangular patterns (lidar, depth), line of sight between point pairs, contact and collision probes, points sampled
 * on surfaces.  Rays, segments and answers live in DEVICE memory; both calls are queued on the context's stream (rtx_set_stream: the
 * caller's) and return at once: nothing is read back, nothing waits, the inputs are read when the work runs and must stay valid until then.
 * The scene is the frame the context holds when the call is made: what rtx_set_frame set, or what rtx_update_instances / rtx_refit_blas /
 * rtx_build_blas last wrote into it.  They work with bounces == 0 and with a frame without lights, and they use a queue set of their own:
 * a query between two render calls changes neither frame, nor what rtx_get_stats reports for them.
 *
 * rtx_query_closest: ray i = rays_dev[6i .. 6i+5] (origin, direction; any 4-byte aligned address) through Scene::trace_primitives
 * (Scene.cpp:173-180: spheres, planes, then the TLAS) by the production closest-hit kernel, its RayHit rebuilt by the functions the shading
 * pass uses (the accept branches of BottomLevelBVH::triangle_trace, Sphere::trace, Plane::trace), with zero ray differentials.  Directions
 * are used as given, distances are in units of |direction|; there is no per-ray tmin / tmax (the reference has none).
 * Channel (bit)          per ray      hit                                                        miss
 *   DISTANCE             f32          RayHit::distance (RayHit.h:6)                              +INFINITY
 *   POSITION             3 x f32      RayHit::point, world space (RayHit.h:8)                     0
 *   NORMAL               3 x f32      RayHit::normal (RayHit.h:9)                                 0
 *   UV                   2 x f32      RayHit::u, v (RayHit.h:12)                                  0
 *   MATERIAL_ID          i32          RayHit::material_id, global (RayHit.h:11)                   -1
 *   OBJECT_ID            i32          the numbering of RTX_AOV_OBJECT_ID                          -1
 *   TRIANGLE_ID          i32          the numbering of RTX_AOV_TRIANGLE_ID                        -1 (also for spheres and planes)
 * The bits are the RTX_AOV_* bits of the same meaning; there is no albedo (no texture is sampled).  A channel is written only if its bit
 * is set and its pointer is not NULL; element i of every written channel belongs to ray i; nothing beyond element n - 1 is touched.
 * Distance and ids come straight from the hit record; position, normal and uv cost the rebuild (two more record reads and, for a
 * triangle, its cold record), which runs only when one of the three is requested.
 * A ray whose direction is exactly (+-0, +-0, +-0) is no ray, as for ray views (rtx_ray above): it is not traced and gets the miss values.
 * Any other floats are legal.  A ray with a NaN or infinite origin or direction component hits nothing in the reference's arithmetic
 * (every hit test ends in a comparison with a NaN, a zero or an infinite distance): it gets the miss values too.
 *
 * rtx_query_occluded: segment i = segments_dev[7i .. 7i+6] (origin, direction, max distance) through Scene::intersect_primitives
 * (Scene.cpp:182-190) by the production shadow-ray kernel: occluded_dev[i] = 1 when something is hit at RAY_EPSILON < t < max distance
 * (strictly, as the reference's shadow rays), else 0.  A zero-direction segment is not occluded; nor is one with a NaN or infinite
 * component, or a maximum distance that is NaN or not above 0.  +INFINITY is a legal maximum distance (a directional light's).
 *
 * Any n >= 1: rays are traced in rounds of at most RTX_QUERY_CHUNK_RAYS, queued back to back, so the scratch (52 bytes per ray of a round:
 * ray, hit and segment records; allocated by the first call, grown only, freed by rtx_destroy) is bounded whatever n is.  A call with the
 * same or a smaller n than an earlier one allocates and frees nothing; one that grows the scratch waits for the stream first.
 * flags: RTX_RENDER_LANE_TRACE / RTX_RENDER_PACKET_CLOSEST choose the kernel as for a render call (the answers are bit-identical);
 * scenes whose trees exceed the packet kernels' limits take the per-lane kernels as in a render call.  A packet is 64 consecutive rays:
 * rays that travel together are cheapest next to each other.
 * RTX_QUERY_SORT (with either of the two, or alone): the library puts the rays of every round into a coherent order itself, on the device,
 * and hands the answers back in the caller's order — for callers who do not choose their row order (lidar beams in firing order, point
 * pairs, contact probes, surface samples).  Per round: the bounds of the rows, a 64-bit key per row (csrc/rtx_query_sort_math.h: a Morton code
 * over the origin and the direction's point on the unit cube, quantised between the round's bounds; rtxh_query_sort_order in rtx_host.h
 * is the same code on the host), rocPRIM's radix sort, the fill gathering rows in sorted order, the same traversal launch, the answers
 * scattered to their rows.  Element i of every channel still belongs to row i, every channel and the occlusion bit are bit-identical to the
 * call without the flag, nothing beyond element n - 1 is touched.  Rows that are not traced (zero direction, a non-finite component, a NaN
 * maximum distance) sort last, so whole packets of them cost nothing.  Rounds are sorted on their own.  The host is not involved and the
 * stream never waits; the flag adds 16 bytes per ray of a round (unsorted and sorted keys) and rocPRIM's temporary storage for a round,
 * allocated by the first sorted call under the rule above — a context that never sorts pays nothing.
 * RTX_ERR_INVALID_ARG: n < 1, NULL rays_dev / segments_dev / out / occluded_dev, channels == 0 or with bits outside RTX_QUERY_ALL, any
 * other flag.  RTX_ERR_STATE: before rtx_set_frame, in heat-map mode, or for a scene a render call refuses (an id outside its table);
 * RTX_ERR_LIMIT: a BVH deeper than rtx_config.stack_size allows — the checks of rtx_render_tiles.  An error queues nothing.
 * Out of scope: sorted rays handed back to the caller, sorting across rounds or ray views, a threshold that sorts by itself, barycentrics,
 * albedo, the rtx_group_* path.                                                                                                          */
enum { RTX_QUERY_DISTANCE = 1, RTX_QUERY_POSITION = 2, RTX_QUERY_NORMAL = 4, RTX_QUERY_UV = 16,
       RTX_QUERY_MATERIAL_ID = 32, RTX_QUERY_OBJECT_ID = 64, RTX_QUERY_TRIANGLE_ID = 128,
       RTX_QUERY_ALL = 247 };            /* the RTX_AOV_* bits of the same meaning; there is no albedo */
enum { RTX_QUERY_CHUNK_RAYS = 1 << 20 }; /* rays traced per internal round */
enum { RTX_QUERY_SORT = 256 };           /* a bit of `flags` of both query calls, next to the RTX_RENDER_* bits they take */
typedef struct rtx_query_buffers {       /* device pointers, one per channel, NULL = not written */
    float   * distance;                  /* [n]     RayHit::distance, +INFINITY on a miss */
    float   * position;                  /* [n][3]  RayHit::point,  0 on a miss            */
    float   * normal;                    /* [n][3]  RayHit::normal, 0 on a miss            */
    float   * uv;                        /* [n][2]  RayHit::u, v,   0 on a miss            */
    int32_t * material_id;               /* [n]     global id, -1 on a miss                */
    int32_t * object_id;                 /* [n]     numbering of RTX_AOV_OBJECT_ID, -1     */
    int32_t * triangle_id;               /* [n]     numbering of RTX_AOV_TRIANGLE_ID, -1   */
} rtx_query_buffers;
int rtx_query_closest (rtx_ctx * ctx, const void * rays_dev /* [n][6] f32: origin, direction */, int64_t n,
                       uint32_t channels, const rtx_query_buffers * out, uint32_t flags);
int rtx_query_occluded(rtx_ctx * ctx, const void * segments_dev /* [n][7] f32: origin, direction, max distance */, int64_t n,
                       int32_t * occluded_dev /* [n]: 1 or 0 */, uint32_t flags);
/* The order RTX_QUERY_SORT traces n rows in, without tracing them: the bounds, key and sort launches of every round, then
 * order_out_dev[first + i] = first + the caller's row in slot i of the round that starts at row `first`.  row_floats: 6 (rays) or 7
 * (segments) or 4 (the points of rtx_query_nearest, below), anything else is RTX_ERR_INVALID_ARG; otherwise queued and checked like the query calls (n beyond INT32_MAX: RTX_ERR_LIMIT). */
int rtx_debug_query_order(rtx_ctx * ctx, const void * rows_dev, int32_t row_floats /* 4, 6 or 7 */, int64_t n, int32_t * order_out_dev);

/* ---- nearest-point queries -------------------------------------------------------------------------------------------------------------
 * "How far is this point from the scene, and where is the nearest surface point": for contact and collision probes, cloth and particle
 * steps, deformations that must stay near a surface.  rtx_query_nearest: row i = points_dev[4i .. 4i+3] = (x, y, z, maximum distance), fp32 at
 * any 4-byte aligned address in DEVICE memory; the scene is the frame the context holds, device-side updates (rtx_update_instances,
 * rtx_refit_blas, rtx_build_blas) included.  Queued on the context's stream, returns at once, nothing is read back; a steady-state call
 * allocates and frees nothing.  Works with bounces == 0 and without lights; touches no queue, frame or counter of a render call.
 * Channels and rtx_query_buffers are those of rtx_query_closest (RTX_QUERY_* bits); a channel is written only if its bit is set and its
 * pointer is not NULL; element i belongs to row i; nothing beyond element n - 1 is touched.
 * Channel                answer                                                                        no answer
 *   DISTANCE             sqrtf of the winning squared distance                                           +INFINITY
 *   POSITION             the nearest surface point, world space                                          0
 *   NORMAL, UV           what RayHit::normal, u, v would hold at that point                              0
 *   MATERIAL_ID, OBJECT_ID, TRIANGLE_ID   the numberings of rtx_query_closest                            -1
 * No answer: nothing lies strictly nearer than the maximum distance; x, y or z is NaN or infinite; the maximum distance is NaN or not above
 * 0; the point is so remote that every squared distance overflows.  +INFINITY is a legal maximum distance.
 * The arithmetic, the order of the walk (which fixes who wins an exact tie) and the accuracy bound are specified in the header comment of
 * csrc/rtx_nearest_math.h; rtxh_query_nearest in rtx_host.h is the same code on the host and gives the same bits.
 * Any n >= 1, in rounds of RTX_QUERY_CHUNK_RAYS rows, one kernel launch per round.  flags: RTX_QUERY_SORT or 0.  With RTX_QUERY_SORT the
 * rows of a round are walked in the Morton order of their points (rows without an answer by rule last, unwalked) and the answers scattered
 * back: bit-identical, row for row; the sort scratch and its growth rule are those of the ray queries.
 * Errors, in this order: RTX_ERR_INVALID_ARG: channels == 0 or with bits outside RTX_QUERY_ALL; a NULL ctx, points_dev or out, n < 1; any
 * flag but RTX_QUERY_SORT.  RTX_ERR_STATE: before rtx_set_frame, in heat-map mode, a scene a render call refuses.  RTX_ERR_LIMIT: a BVH
 * deeper than rtx_config.stack_size allows (the check of rtx_render_tiles).  RTX_ERR_STATE: the rigid rule — a frame with an instance
 * whose matrix is not a rigid pose (Limits, below).  RTX_ERR_LIMIT: the walk's own stack rule: it holds at most (TLAS inner
 * depth + 1) + (deepest BLAS inner depth + 1) entries (inner depth: that of the deepest inner node, root 0; -1 for a single leaf), and a
 * scene that needs more than rtx_config.stack_size is refused.  An error queues nothing.
 * Limits: distances are measured in each instance's LOCAL space, and the walk prunes by WORLD-space box distances: the two agree only for
 * rigid poses.  The rigid rule: rtx_set_frame judges every instance it is handed — rigid iff, for the linear parts R of both world and
 * world_inv, every |(R.R^T - I)ij| <= 2^-12, in fp64 (a reflection passes; rtxh_instances_rigid in rtx_host.h is the same code) — and a frame
 * with a scaled, sheared or flattened instance is refused by this call, by rtx_query_signed_distance, rtx_query_sweep, rtx_query_overlap, rtx_query_overlap_capsule and
 * rtx_query_sweep_box and by their _filtered forms (before this rule such a frame lost answers: the walk pruned a scaled instance by a
 * bound in its local units).  rtx_query_hits, rtx_query_closest, rtx_query_occluded and the render calls take any finite matrix: t does not
 * change under an affine map.  After rtx_update_instances the frame counts as rigid, by that call's unit-quaternion contract.  For the
 * poses Mesh::update makes from unit quaternions the local metric is the world metric up to rounding; a matrix within the 2^-12 but
 * farther from orthogonal than those adds 2^-13 times the distance to the bounds stated for these queries.  The
 * answer may depend on the tree within the bound: a refit, or a rebuild of the same triangles, may return another triangle at an equal
 * or nearly equal distance.  The side of the surface: rtx_query_signed_distance, below.  Out of scope: k nearest, all within a radius,
 * barycentrics, the rtx_group_* path.                                                                                                    */
int rtx_query_nearest(rtx_ctx * ctx, const void * points_dev /* [n][4] f32: x, y, z, maximum distance */, int64_t n,
                      uint32_t channels, const rtx_query_buffers * out, uint32_t flags);

/* ---- all-hits segment queries ----------------------------------------------------------------------------------------------------------
 * "Everything this segment crosses": the nearest max_hits hits of every row in order, and how many there were.  For inside / outside by
 * crossing parity (the sign of the distance in one call, open surfaces included: rtx_query_signed_distance), thickness and penetration depth as entry / exit pairs, multi-echo
 * lidar and depth peeling (the 2nd, 3rd, ... return), the number of surfaces between two points.  rtx_query_hits: row i =
 * segments_dev[7i .. 7i+6] = (origin, direction, max distance D), the rows of rtx_query_occluded, fp32 at any 4-byte aligned address in
 * DEVICE memory; the scene is the frame the context holds, device-side updates included.  Queued on the context's stream, returns at once,
 * nothing is read back; a steady-state call allocates and frees nothing.  Works with bounces == 0 and without lights; touches no queue,
 * frame or counter of a render call.
 * A hit is anything the reference's own tests accept at RAY_EPSILON < t < D, every comparison strict: tri_test in the instance's local ray,
 * Plane::trace's distance, and BOTH roots of Sphere::trace's quadratic (a ray through a sphere crosses it twice; a tangent gives two equal
 * hits).  t is in units of |direction|.  Hits are ordered by (t, object_id, triangle_id) ascending.
 * Channels are the RTX_QUERY_* bits and rtx_query_buffers is reused with stride K = max_hits: hit j of row i is element i*K + j of every
 * written channel (times 3 or 2 for the vector channels); a channel is written only if its bit is set and its pointer is not NULL; nothing
 * beyond row n - 1 is touched.  Position, normal, uv and material of a hit are what rtx_query_closest would report had that hit been the
 * closest (the accept branches of the shading pass at that t, zero differentials).  Entries j >= min(count, K) hold the miss values of
 * rtx_query_closest: +INFINITY, 0, -1.
 * count_dev[i] (may be NULL) = the number of hits of row i; it may exceed K.  max_hits == 0 with channels == 0 and a non-NULL count_dev is the
 * count-only form: no list is kept.  Otherwise 1 <= max_hits <= RTX_QUERY_MAX_HITS and channels != 0.
 * A dead row — a zero direction, a NaN or infinite component, a D that is NaN or not above 0 — is not walked: count 0, miss values.
 * +INFINITY is a legal D.
 * The arithmetic, the order and the walk are specified in the header comment of csrc/rtx_hits_math.h; rtxh_query_hits in rtx_host.h is the
 * same code on the host and gives the same bits.  Promised: every listed hit is a hit of the exhaustive search over all primitives, with the
 * same bits, and count <= the exhaustive count.  Not promised: equality with the exhaustive list on every row — the reference's box test can
 * reject a box whose triangle its triangle test accepts (a flat box, a box plane within an ulp of the hit), as for rtx_query_closest.  When
 * no count is requested the box tests use the K-th hit's distance once the list is full; lists with and without a count may then differ on
 * rows with such hits or with a hit exactly as far as the K-th.
 * Any n >= 1, in rounds of RTX_QUERY_CHUNK_RAYS rows, one kernel launch per round.  flags: RTX_QUERY_SORT or 0; with it the rows of a round are
 * walked in the order of the ray queries' 7-float keys and the answers scattered back: bit-identical, row for row.
 * Errors, in this order: RTX_ERR_INVALID_ARG: a max_hits / channels / count_dev combination other than the two above, channels outside
 * RTX_QUERY_ALL; a NULL ctx or segments_dev, a NULL out (a NULL count_dev in the count-only form), n < 1; any flag but RTX_QUERY_SORT.
 * RTX_ERR_STATE and RTX_ERR_LIMIT: as for rtx_query_nearest, its stack rule included and its rigid rule left out (t does not change under an
 * affine map: any finite matrix is served).  An error queues nothing.
 * Limits: a BLAS whose leaves share triangles (the reference's SBVH with spatial splits) holds such a triangle once per slot, and every slot
 * is a hit.  Out of scope: hits beyond RTX_QUERY_MAX_HITS per row, an any-hit callback or per-material filtering (whole objects are
 * hidden by mask: filtered queries, below), a per-ray tmin other than RAY_EPSILON, signed distance as a single call, barycentrics as a channel, the rtx_group_* path.                                   */
enum { RTX_QUERY_MAX_HITS = 8 };
int rtx_query_hits(rtx_ctx * ctx, const void * segments_dev /* [n][7] f32: origin, direction, max distance */, int64_t n,
                   int32_t max_hits /* K */, uint32_t channels, const rtx_query_buffers * out /* each channel [n][K] */,
                   int32_t * count_dev /* [n] or NULL */, uint32_t flags /* RTX_QUERY_SORT or 0 */);

/* ---- swept-sphere queries --------------------------------------------------------------------------------------------------------------
 * "How far can this ball travel along this direction before it touches something, and where does it touch": a particle with a radius, a
 * collision proxy, a camera boom, a thick lidar beam, a conservative-advancement step.  rtx_query_sweep: row i = sweeps_dev[8i .. 8i+7] =
 * (origin, direction, max distance D, radius r), fp32 at any 4-byte aligned address in DEVICE memory; the scene is the frame the context
 * holds, device-side updates included.  Queued on the context's stream, returns at once, nothing is read back; a steady-state call allocates
 * and frees nothing.  Works with bounces == 0 and without lights; touches no queue, frame or counter of a render call.
 * The ball's centre moves along c(t) = origin + t * direction, the direction used as given, t in units of |direction|; r is in world units.
 * The answer is the smallest t in [0, D) (D itself excluded) at which the distance from c(t) to the surface rtx_query_nearest measures —
 * two-sided triangles, sphere shells (a ball inside a large sphere travels until it touches the shell from inside), two-sided planes — is
 * <= r.  A ball that touches something at its origin answers t = 0 with the primitive and the surface point rtx_query_nearest reports for
 * (origin, r): candidates are ordered by (t, squared distance from the origin), an exact tie goes to the lowest (kind, object, slot).
 * A dead row — a zero direction, a NaN or infinite origin or direction component, a D that is NaN or not above 0, an r that is NaN, infinite
 * or not above 0 — is not walked and gets the no-answer values.  +INFINITY is a legal D.
 * Channels and rtx_query_buffers are those of rtx_query_closest; a channel is written only if its bit is set and its pointer is not NULL;
 * element i belongs to row i; nothing beyond row n - 1 is touched.
 * Channel                answer                                                                        no answer
 *   DISTANCE             t                                                                               +INFINITY
 *   POSITION             the contact point on the surface, world space                                   0
 *   NORMAL, UV           what rtx_query_nearest reports for that surface point                           0
 *   MATERIAL_ID, OBJECT_ID, TRIANGLE_ID   the numberings of rtx_query_closest                            -1
 * NORMAL is the surface's shading normal.  The geometric contact normal is (c(t) - position) / r; there is no channel for it.
 * The arithmetic, the order of the walk and the accuracy bound (stated in distance: for the returned t the distance from c(t) to the
 * returned primitive is within the bound of r, and nothing is nearer than r minus the bound before t) are specified in the header comment
 * of csrc/rtx_sweep_math.h; rtxh_query_sweep in rtx_host.h is the same code on the host and gives the same bits.
 * Any n >= 1, in rounds of RTX_QUERY_CHUNK_RAYS rows, one kernel launch per round.  flags: RTX_QUERY_SORT or 0; with it the rows of a round are
 * walked in the order of the ray queries' 7-float keys, taken over each row's first seven floats, and the answers scattered back:
 * bit-identical, row for row.
 * Errors, in this order and with the codes of rtx_query_nearest, its rigid rule and its stack rule included.  An error queues nothing.
 * Limits: r and the distances are measured in each instance's LOCAL space, as for rtx_query_nearest — the world metric for rigid poses; a
 * frame with a scaled, sheared or flattened instance is refused (the rigid rule of rtx_query_nearest).  The answer may depend on the tree within the bound.  Out of scope: swept capsules or rotating shapes (a
 * swept box is rtx_query_sweep_box), all contacts along the sweep, a contact-normal channel, the rtx_group_* path.                                                    */
int rtx_query_sweep(rtx_ctx * ctx, const void * sweeps_dev /* [n][8] f32: origin, direction, max distance, radius */, int64_t n,
                    uint32_t channels, const rtx_query_buffers * out, uint32_t flags /* RTX_QUERY_SORT or 0 */);

/* ---- filtered queries: object masks -----------------------------------------------------------------------------------------------------
 * "Each row sees only some objects": a cloth vertex that must not find its own mesh, a ball swept from a robot's link that must not touch
 * that link, a lidar on a body, a line of sight between two objects — while the body stays part of the one frame that is also rendered.
 * The instance / layer masks of other ray-query interfaces, for the three walk queries above.
 * Objects are numbered as RTX_AOV_OBJECT_ID numbers them: instance i -> i, sphere s -> I + s, plane p -> I + S + p; M = I + S + P.
 * Object masks: a table of M uint32_t owned by the context; without a table every object's mask is 0xFFFFFFFF.
 * Row masks: one uint32_t per row, from the device array rtx_query_filter.row_masks_dev[n], or the scalar row_mask for every row when that
 * pointer is NULL.
 * Rule: an object exists for a row iff (object_mask & row_mask) != 0.  A hidden sphere or plane is not offered as a candidate; a hidden
 * instance is passed over where the walk takes it from its TLAS leaf, before its matrix or its BLAS is touched; nothing else in the walk
 * changes (TLAS boxes still contain hidden instances; order, tie rules and the stack rule are the same): FILTER in the header comment of
 * csrc/rtx_nearest_math.h.  rtx_query_hits neither lists nor counts a hidden object; for rtx_query_sweep it neither stops the ball nor
 * overlaps it.  A row whose mask is 0 is answered without a walk: the no-answer values, count 0.  The accuracy bounds of the three queries
 * and what rtx_query_hits promises hold unchanged against the exhaustive search over the visible primitives; the rtxh_*_filtered functions
 * of rtx_host.h are the same code on the host and give the same bits.
 *
 * rtx_set_object_masks copies count masks from HOST memory (through a pinned staging ring, one copy on the context's stream: a query queued
 * before the call reads the old table, one queued after it the new).  rtx_update_object_masks copies them from DEVICE memory on the stream:
 * nothing is read back, no pointer changes.  The table's allocation only grows (a call that grows it waits for the stream first); a
 * steady-state call allocates nothing.  rtx_read_object_masks waits for the stream and reads back what the kernels see: *count = the
 * table's length (0: no table), out[0 .. *count) if out is not NULL.
 * Errors of the three, in this order: a NULL ctx: RTX_ERR_INVALID_ARG.  Before rtx_set_frame: RTX_ERR_STATE.  NULL masks with count 0 drops
 * the table (its memory is kept).  Otherwise count must equal M of the current frame and masks must not be NULL (masks_dev 4-byte aligned):
 * RTX_ERR_INVALID_ARG.  rtx_read_object_masks: out and count both NULL, capacity < 0 or below the table's length: RTX_ERR_INVALID_ARG.
 * The context remembers (I, S, P) as they were when the table was set.  A later rtx_set_frame keeps the table; rtx_update_instances,
 * rtx_refit_blas and rtx_build_blas do not touch it.  A filtered query whose frame has other counts than the remembered ones is
 * RTX_ERR_STATE and queues nothing: set the masks again, or drop them.
 *
 * rtx_query_nearest_filtered, rtx_query_hits_filtered, rtx_query_sweep_filtered: the arguments, channels, flags, errors (in their order) and
 * every rule of the call without the suffix, plus the filter; after those errors, the state rule above.  A NULL filter IS the call without
 * the suffix: the same kernel, the same bits.  A filter without a table and with row_mask 0xFFFFFFFF, or with a table of all ones and row masks
 * of all ones, gives the unfiltered answers bit for bit (by another kernel instantiation).  With RTX_QUERY_SORT the mask of slot i is that
 * of the caller's row in that slot, gathered like the row itself; the sort key does not know the masks; answers are bit-identical, row for
 * row, to the unsorted filtered call.  row_masks_dev is read during the call's kernels: keep it alive and unchanged until they have run.
 * rtx_query_closest and rtx_query_occluded run on the render path's traversal kernels and stay unfiltered: a filtered closest hit is
 * rtx_query_hits_filtered with max_hits = 1 (its one listed hit is the closest visible one), a filtered occlusion test its count-only
 * form (count > 0).
 * Out of scope: filtering in rtx_query_closest, rtx_query_occluded and render calls; exclusion by object or triangle id; per-material
 * filtering; skipping the triangles next to a vertex (self-collision within one object); a per-ray tmin; the rtx_group_* path.             */
typedef struct rtx_query_filter {
    const uint32_t * row_masks_dev;      /* [n] in device memory, or NULL: row_mask for every row */
    uint32_t row_mask;
} rtx_query_filter;
int rtx_set_object_masks(rtx_ctx * ctx, const uint32_t * masks_host /* [count] */, int32_t count /* M, or 0 with NULL */);
int rtx_update_object_masks(rtx_ctx * ctx, const void * masks_dev /* [count] u32 */, int32_t count);
int rtx_read_object_masks(rtx_ctx * ctx, uint32_t * out /* [capacity] or NULL */, int32_t capacity, int32_t * count);
int rtx_query_nearest_filtered(rtx_ctx * ctx, const void * points_dev, int64_t n, uint32_t channels, const rtx_query_buffers * out, uint32_t flags,
                               const rtx_query_filter * filter);
int rtx_query_hits_filtered(rtx_ctx * ctx, const void * segments_dev, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                            int32_t * count_dev, uint32_t flags, const rtx_query_filter * filter);
int rtx_query_sweep_filtered(rtx_ctx * ctx, const void * sweeps_dev, int64_t n, uint32_t channels, const rtx_query_buffers * out, uint32_t flags,
                             const rtx_query_filter * filter);

/* ---- signed-distance queries ------------------------------------------------------------------------------------------------------------
 * "On which side of the surface is this point": rtx_query_nearest with a sign.  rtx_query_signed_distance walks the rows exactly as
 * rtx_query_nearest / rtx_query_nearest_filtered do (filter NULL: unfiltered) and writes the channels of the same call bit for bit — channels
 * may be 0, and then out may be NULL — plus signed_dev[i] (required): the distance of row i, NEGATIVE iff r . N < 0, where r is the vector
 * from the nearest surface point to the row's point and N the pseudonormal of the feature of the nearest triangle that holds that point: the
 * face normal e1 x e2 of the slot, the edge's or the vertex's record of the tables rtx_blas_pseudonormals made.  r . N == 0, a zero N and a
 * NaN are positive; a point on the surface gets +0.  Both vectors are in the instance's local space, so rigid and mirrored instances
 * need nothing more (a scaled one is refused: the rigid rule of rtx_query_nearest).  A sphere is negative inside (l < r with the two roots of its distance), a plane where n.p + distance < 0.  A row
 * without an answer gets +INFINITY.  feature_dev[i] (or NULL): 0 none, 1 face, 2 edge, 3 vertex, 4 sphere, 5 plane; + 8 when the winning
 * mesh has no tables — then e1 x e2 is used in every region, the naive rule, which is wrong near convex and concave edges and vertices.
 * For a closed, consistently oriented mesh negative is inside; for an open one it is the side the orientation calls back.  The sign rule is
 * specified in the header comment of csrc/rtx_side_math.h (SIDE, FEATURE, LIMITS); rtxh_query_signed_distance in rtx_host.h gives the same
 * bits.  One launch per round, the walk's kernel; after the walk the winner's matrix and three 16-byte hot loads, the region chain, then the
 * mesh's 32-byte table entry and, behind it, one record (an edge) or a slot vertex and its record (a vertex): up to three dependent loads.
 * Errors, in this order: RTX_ERR_INVALID_ARG: a NULL ctx; channels with bits outside RTX_QUERY_ALL; a NULL or misaligned signed_dev, a
 * misaligned feature_dev; a NULL points_dev, a NULL out with channels != 0, n < 1; any flag but RTX_QUERY_SORT.  Then RTX_ERR_STATE and
 * RTX_ERR_LIMIT as for rtx_query_nearest, its rigid rule and its stack rule included, and the state rule of the filtered queries.  An error queues nothing.
 * Limits: the sign is relative to the OBJECT that owns the nearest point — for overlapping solids it is not the sign of their union.  Within
 * the accuracy bound of rtx_query_nearest of a surface, and where r is within rounding of perpendicular to N, the sign is not determined.
 * Out of scope: signed sweeps, generalized winding numbers, the sign of a union, the rtx_group_* path.                                    */
int rtx_query_signed_distance(rtx_ctx * ctx, const void * points_dev /* [n][4] f32 */, int64_t n, uint32_t channels /* may be 0 */,
                              const rtx_query_buffers * out /* may be NULL iff channels == 0 */, float * signed_dev /* [n], required */,
                              int32_t * feature_dev /* [n] or NULL */, uint32_t flags /* RTX_QUERY_SORT or 0 */,
                              const rtx_query_filter * filter /* NULL: unfiltered */);

/* ---- box-overlap queries ----------------------------------------------------------------------------------------------------------------
 * "What does this volume touch": a collision proxy (is this oriented box free), a trigger volume or broad phase (which objects are in this
 * region), voxelisation (one box per voxel: occupancy, conservative voxelisation, surface-voxel counts), a gather (which triangles lie under
 * this footprint).  rtx_query_overlap: row i = boxes_dev[10i .. 10i+9] = (centre c, half extents h, rotation quaternion x, y, z, w — the
 * convention of rtx_update_instances; normalised by the library).  A row is live when all ten floats are finite, every half extent is >= 0
 * (zero is allowed: a point, a segment, a rectangle) and the quaternion is not zero; a dead row overlaps nothing.  Surfaces are what the
 * query family measures everywhere: a triangle overlaps by the 13-axis separating-axis test (touching is overlapping), a sphere when its
 * shell meets the box (a box strictly inside the ball does not overlap), a plane when the box reaches it.  Everything is specified in the
 * header comment of csrc/rtx_overlap_math.h (ROW, TRIANGLE, SPHERE, PLANE, NODE, ORDER, WALK, FORMS, MARGIN, PROMISED); rtxh_query_overlap in
 * rtx_host.h gives the same bits.  Like rtx_query_nearest the test runs in each instance's local frame: exact for rigid poses, and a frame
 * with an instance that is not one is refused (the rigid rule of rtx_query_nearest).
 * Three forms, chosen by flags:
 *   0                      the (object, triangle slot) overlaps of every row, ordered by (object_id, triangle_id) ascending — object ids in
 *                          the numbering of RTX_QUERY_OBJECT_ID, triangle_id -1 for spheres and planes: object_id_dev / triangle_id_dev
 *                          [n][max_hits] hold the max_hits smallest (either may be NULL), entries past the count -1; count_dev[n] (or NULL)
 *                          the number of all overlaps of the row, which may exceed max_hits.
 *   RTX_OVERLAP_OBJECTS    the distinct objects: an instance counts once, however many of its triangles overlap.  triangle_id_dev must be NULL.
 *   RTX_OVERLAP_ANY        count_dev[i] = 1 if anything overlaps, else 0; the walk of a row ends at its first overlap.  max_hits must be 0.
 * max_hits in [0, RTX_QUERY_MAX_HITS]; max_hits == 0 is the count-only form and needs count_dev; max_hits > 0 needs at least one id array.
 * Any n >= 1, in rounds of RTX_QUERY_CHUNK_RAYS rows, one kernel launch per round.  RTX_QUERY_SORT: the rows of a round are walked in the
 * Morton order of their centres (the position key of rtx_query_nearest over the first three floats of a row); the answers come back in the
 * caller's order, bit for bit those of the unsorted call.  The call runs on the context's stream; nothing is read back, frames, render calls
 * and rtx_get_stats are unchanged.  rtx_query_overlap_filtered: the same with the object masks of the filtered queries above — a hidden
 * object is neither listed nor counted, a row whose mask is 0 overlaps nothing.
 * Errors, in this order: RTX_ERR_INVALID_ARG: a NULL ctx; max_hits outside [0, RTX_QUERY_MAX_HITS]; RTX_OVERLAP_ANY with max_hits != 0 or
 * with RTX_OVERLAP_OBJECTS; RTX_OVERLAP_OBJECTS with a triangle_id_dev; max_hits == 0 without a count_dev; max_hits > 0 without an id array;
 * a NULL boxes_dev, n < 1; any flag but RTX_QUERY_SORT, RTX_OVERLAP_OBJECTS, RTX_OVERLAP_ANY.  Then RTX_ERR_STATE and RTX_ERR_LIMIT as for
 * rtx_query_nearest, its rigid rule and its stack rule included, and the state rule of the filtered queries.  An error queues nothing.
 * Out of scope: convex hulls as query volumes (capsules and balls: rtx_query_overlap_capsule), penetration depth (a swept box is rtx_query_sweep_box), or contact points, more than
 * RTX_QUERY_MAX_HITS entries per row, the rtx_group_* path.                                                                              */
enum { RTX_OVERLAP_OBJECTS = 512, RTX_OVERLAP_ANY = 1024 };      /* bits of rtx_query_overlap's flags, beside RTX_QUERY_SORT */
int rtx_query_overlap(rtx_ctx * ctx, const void * boxes_dev /* [n][10] f32: centre, half extents, quaternion */, int64_t n, int32_t max_hits,
                      int32_t * object_id_dev /* [n][max_hits] or NULL */, int32_t * triangle_id_dev /* [n][max_hits] or NULL */,
                      int32_t * count_dev /* [n] or NULL */, uint32_t flags /* RTX_QUERY_SORT, RTX_OVERLAP_OBJECTS, RTX_OVERLAP_ANY or 0 */);
int rtx_query_overlap_filtered(rtx_ctx * ctx, const void * boxes_dev, int64_t n, int32_t max_hits, int32_t * object_id_dev, int32_t * triangle_id_dev,
                               int32_t * count_dev, uint32_t flags, const rtx_query_filter * filter);

/* ---- capsule-overlap queries ------------------------------------------------------------------------------------------------------------
 * "What does this capsule or ball touch": a character, a robot link or a finger with a capsule proxy, a cable or cloth edge with a
 * thickness, a particle with a radius (every primitive within r of a point: the within-radius gather).
 * rtx_query_overlap_capsule: row i = capsules_dev[7i .. 7i+6] = (start point p, axis vector d, radius r), fp32 at any 4-byte aligned
 * address in DEVICE memory: the capsule is every point within r of the segment p + s d, s in [0, 1] — the first seven floats of a
 * rtx_query_sweep row with d = direction * D.  A row is live when all seven floats are finite and r >= 0; d == 0 is a ball, r == 0 a
 * segment, both a point; a dead row overlaps nothing.  A triangle overlaps iff its distance to the segment is <= r (touching is
 * overlapping), a sphere when its shell meets the capsule (a capsule strictly inside the ball does not overlap), a plane when the capsule
 * reaches it.  Everything is specified in the header comment of csrc/rtx_capsule_math.h (ROW, FRAME, TRIANGLE, SPHERE, PLANE, NODE, ORDER,
 * WALK, FORMS, FILTER, MARGIN, PROMISED); rtxh_query_overlap_capsule in rtx_host.h gives the same bits.
 * The forms, flags, outputs, max_hits rules and rounds are those of rtx_query_overlap.  RTX_QUERY_SORT: the rows of a round are walked in
 * the order of the ray key of rtx_query_closest over (p, d); a ball row (d == 0) has no ray key: it sorts with the dead rows, last, and is
 * walked all the same.  The call runs on the context's stream; nothing is read back, frames, render calls and rtx_get_stats are unchanged.
 * rtx_query_overlap_capsule_filtered: the same with the object masks of the filtered queries above; a NULL filter is the unfiltered call.
 * Errors: those of rtx_query_overlap in its order (capsules_dev for boxes_dev), its rigid rule and its stack rule included.
 * Out of scope: swept capsules, a contact point or penetration depth, a position sort key for ball-only batches, more than
 * RTX_QUERY_MAX_HITS entries per row, the rtx_group_* path.                                                                              */
int rtx_query_overlap_capsule(rtx_ctx * ctx, const void * capsules_dev /* [n][7] f32: p, d, r */, int64_t n, int32_t max_hits,
                              int32_t * object_id_dev /* [n][max_hits] or NULL */, int32_t * triangle_id_dev /* [n][max_hits] or NULL */,
                              int32_t * count_dev /* [n] or NULL */, uint32_t flags /* RTX_QUERY_SORT, RTX_OVERLAP_OBJECTS, RTX_OVERLAP_ANY or 0 */);
int rtx_query_overlap_capsule_filtered(rtx_ctx * ctx, const void * capsules_dev, int64_t n, int32_t max_hits, int32_t * object_id_dev, int32_t * triangle_id_dev,
                                       int32_t * count_dev, uint32_t flags, const rtx_query_filter * filter);

/* ---- swept-box queries ------------------------------------------------------------------------------------------------------------------
 * "How far can this oriented box travel along this direction before it touches something, what does it touch, and with which face or edge":
 * a character controller, a vehicle footprint, a gripper finger, a robot link with a box proxy, a pallet on a conveyor.
 * rtx_query_sweep_box: row i = sweeps_dev[14i .. 14i+13] = (centre c, direction d, max distance D, half extents h, rotation quaternion
 * x, y, z, w — the box of rtx_query_overlap, moved without turning), fp32 at any 4-byte aligned address in DEVICE memory; the scene is the
 * frame the context holds, device-side updates included.  Queued on the context's stream, returns at once, nothing is read back; a
 * steady-state call allocates and frees nothing; frames, render calls and rtx_get_stats are unchanged.
 * The box's centre moves along c(t) = c + t * d, d used as given, t in units of |d|.  The answer is the smallest t in [0, D) (D excluded) at
 * which the box touches a surface of the query family: a two-sided triangle by the continuous form of rtx_query_overlap's 13-axis test, a
 * sphere's shell (a box inside a large sphere travels until its farthest corner reaches the shell), a two-sided plane (approached only).  A box
 * that touches something where it starts answers t = 0.  An exact tie in t goes to the lowest (object_id, triangle_id).
 * A row is live when its first seven floats are a live row of rtx_query_sweep's (a direction that is not zero, finite centre and direction,
 * D > 0, +INFINITY included) and (c, h, q) is a live box of rtx_query_overlap (finite, h >= 0 — zero allowed: a point box is a ray — and a
 * quaternion that is not zero).  A dead row is not walked and gets the no-answer values.
 * Outputs, each a caller-supplied device array or NULL, at least one not NULL; element i belongs to row i:
 *   array                   answer                                                                       no answer
 *   t_dev [n] f32           t                                                                            +INFINITY
 *   normal_dev [n][3] f32   the unit contact normal, world space, opposing the motion; 0 where t == 0    0
 *   object_id_dev [n] i32   the numbering of RTX_QUERY_OBJECT_ID                                         -1
 *   triangle_id_dev [n] i32 the triangle's slot in its BLAS; -1 for a sphere or a plane                  -1
 *   axis_dev [n] i32        0..2 a box face's axis, 3 the triangle's normal (a box corner or edge onto   -1
 *                           its face), 4..12 box axis (k - 4) % 3 x triangle edge (k - 4) / 3 (edges: e1,
 *                           e2 - e1, e2): edge against edge; 13 an overlap at t == 0; 14 a sphere; 15 a plane
 * The candidate functions, the order rule, the walk, the slack of its node test and the accuracy bound (stated in distance: at the returned
 * t the returned primitive's largest separating gap is within the bound of 0, and nothing penetrates deeper than the bound before t) are
 * specified in the header comment of csrc/rtx_boxsweep_math.h; rtxh_query_sweep_box in rtx_host.h is the same code on the host and gives the
 * same bits.  Like rtx_query_overlap the test runs in each instance's local frame: exact for rigid poses; other frames are refused.
 * Any n >= 1, in rounds of RTX_QUERY_CHUNK_RAYS rows, one kernel launch per round.  flags: RTX_QUERY_SORT or 0; with it the rows of a round are
 * walked in the order of the ray queries' 7-float keys, taken over each row's first seven floats, and the answers scattered back:
 * bit-identical, row for row.  rtx_query_sweep_box_filtered: the same with the object masks of the filtered queries above and their state
 * rule — a hidden object neither stops the box nor overlaps it, a row whose mask is 0 gets the no-answer values without a walk; a NULL filter
 * is the unfiltered call.
 * Errors, in this order: RTX_ERR_INVALID_ARG: a NULL ctx; a NULL sweeps_dev, five NULL outputs, n < 1; any flag but RTX_QUERY_SORT.  Then
 * RTX_ERR_STATE and RTX_ERR_LIMIT as for rtx_query_nearest, its rigid rule and its stack rule included, and the state rule of the filtered
 * queries.  An error queues nothing.
 * Out of scope: contact points or manifolds, rotation during the sweep, capsules and hulls, all contacts along the path, the rtx_group_* path. */
int rtx_query_sweep_box(rtx_ctx * ctx, const void * sweeps_dev /* [n][14] f32: centre, direction, max distance, half extents, quaternion */, int64_t n,
                        float * t_dev /* [n] or NULL */, float * normal_dev /* [n][3] or NULL */, int32_t * object_id_dev /* [n] or NULL */,
                        int32_t * triangle_id_dev /* [n] or NULL */, int32_t * axis_dev /* [n] or NULL */, uint32_t flags /* RTX_QUERY_SORT or 0 */);
int rtx_query_sweep_box_filtered(rtx_ctx * ctx, const void * sweeps_dev, int64_t n, float * t_dev, float * normal_dev, int32_t * object_id_dev,
                                 int32_t * triangle_id_dev, int32_t * axis_dev, uint32_t flags, const rtx_query_filter * filter);

/* Timing of every kernel launched since rtx_enable_kernel_timing(ctx, 1),
 * measured with HIP events on the stream the kernels are launched on.
 * names/ms hold up to `capacity` entries; *count receives the number of
 * kernel launches recorded.                                                    */
int rtx_last_kernel_times(rtx_ctx * ctx, const char ** names, float * ms, int32_t capacity, int32_t * count);
int rtx_enable_kernel_timing(rtx_ctx * ctx, int32_t enable);

/* ---- several GPUs of one node (BASELINE configs[3]) ------------------------------------------------------
 * The reference hands 32x32 screen tiles to worker threads through an atomic counter (WorkerThread.cpp:53-65,
 * 116-129); tiles are independent given the read-only Scene.  A GPU group does the same across GPUs: tile t
 * belongs to rank t mod world, every rank renders its tiles into a TILE-MAJOR buffer of packed pixels (edge
 * tiles padded to 32x32), ONE RCCL gather per frame moves those buffers to rank 0 over xGMI, and rank 0 writes
 * them into its packed framebuffer (rtx_read_framebuffer / rtx_framebuffer_device_ptrs on rank 0's context).
 * Every rank uploads the same scene and calls rtx_set_frame with the same frame (Scene::update runs on every
 * host, or its result is sent: < 4 KiB).  All calls of a group are collective: every rank makes them in the
 * same order.  RCCL (librccl.so.1) is loaded at run time; without it these functions return RTX_ERR_STATE.   */
typedef struct rtx_group rtx_group;
#define RTX_GROUP_ID_BYTES 128
/* rank 0: a fresh communicator id (ncclGetUniqueId) to hand to the other ranks by any out-of-band channel */
int rtx_group_unique_id(void * id128);
/* one context per process: rank `rank` of `world` joins the group (id128 may be NULL when world == 1) */
int rtx_group_create(rtx_ctx * ctx, int32_t rank, int32_t world, const void * id128, rtx_group ** out_group);
/* this rank's share of one frame + gather + (rank 0) frame assembly; queued on the context's stream, returns at once.
 * flags as rtx_render_tiles (RTX_RENDER_SERIAL is implied).  rtx_get_stats afterwards covers this rank's tiles. */
int rtx_group_render(rtx_group * group, uint32_t flags);
int rtx_group_destroy(rtx_group * group);
/* several frames in flight on one GPU (one context each, as bench.py runs them): the further contexts JOIN the first one's communicator
 * as the same rank instead of opening their own.  The gathers of all members are then issued on one exchange stream per rank in call
 * order (events tie them to the frames' own streams), so every rank issues its collectives in the same order whatever order its frames
 * finish in, and a rank never has two collectives in flight.  Every rank must call rtx_group_render on its members in the same order. */
int rtx_group_attach(rtx_ctx * ctx, rtx_group * base, rtx_group ** out_group);
/* one process driving n GPUs, contexts[i] on its own device = rank i (ncclCommInitAll); render issues all ranks' calls */
int rtx_group_create_local(rtx_ctx ** contexts, int32_t n, rtx_group ** out_groups);
int rtx_group_render_local(rtx_group ** groups, int32_t n, uint32_t flags);
/* The partition and the tile-major slot order as plain host functions (no GPU, no context): the same code the kernels run.
 * rank `rank` of `world` owns tiles rank, rank + world, ... (numbering of WorkerThread.cpp:57-61: the reference hands those task
 * numbers to its threads through an atomic counter, :53-65); every rank sends tiles_per_rank tiles of 1024 packed pixels.
 * rtx_group_slot_pixels: pixel_index[i] = y * width + x of slot i of the rank's send buffer, -1 for padding; rank 0 receives the
 * send buffers concatenated in rank order.  capacity >= tiles_per_rank * 1024. */
int rtx_group_layout(int32_t width, int32_t height, int32_t world, int32_t rank, int32_t * tiles_total, int32_t * tiles_per_rank, int32_t * own_tiles);
int rtx_group_slot_pixels(int32_t width, int32_t height, int32_t world, int32_t rank, int64_t * pixel_index, int64_t capacity);

/* ---- unit-level entry points: one reference function each, evaluated on the device -------------
 * (used by the parity tests; not needed by a renderer)                                          */

/* fn: 0 acosf(a) 1 atan2f(a,b) 2 expf(a) 3 log2f(a) 4 atanf(a) 5 Util::float_to_int(a) = cvtss2si 6 1/sqrtf(a) 7 (int)a = cvttss2si
 * 8 Math::pow2<128>(a), n values each; 5 and 7 return the integer as a float (exact: 24 significant bits at most, the indefinite value
 * is -2^31).  Any other fn: RTX_ERR_INVALID_ARG, nothing allocated or launched. */
int rtx_debug_libm(rtx_ctx * ctx, int32_t fn, const float * a, const float * b, float * out, int32_t n);
/* Texture::sample (Texture.h:33-49) of an uploaded texture at n inputs (s,t,ds_dx,ds_dy,dt_dx,dt_dy) */
int rtx_debug_texture_sample(rtx_ctx * ctx, int32_t texture_id, const float * in6, float * out_rgb, int32_t n);
/* Scene::trace_primitives (Scene.cpp:173-180) of n rays (18 floats each: origin, direction, dO_dx, dO_dy, dD_dx, dD_dy) in host memory
 * through the production closest-hit kernel + the accept-branch rebuild of the shade kernel; out: 27 floats per ray = every RayHit field
 * (RayHit.h:5-21): hit, distance, point[3], normal[3], material_id, u, v, ds_dx, ds_dy, dt_dx, dt_dy, dO_dx[3], dO_dy[3], dN_dx[3], dN_dy[3]
 * (a miss: hit 0, distance +INFINITY, everything else 0).  The call uploads the rays, runs the rounds of rtx_query_closest (above), waits
 * and copies back; rtx_debug_occluded does the same through the rounds of rtx_query_occluded.  So, for both hooks:
 *  - a row with an all-zero direction or a NaN / infinite origin or direction component is not walked and answers as a miss / not
 *    occluded (0): the queries' rule, above;
 *  - flags: RTX_RENDER_LANE_TRACE / RTX_RENDER_PACKET_CLOSEST choose the kernel as for a query, so scenes whose trees exceed the packet
 *    kernels' limits take the per-lane kernels (the answers are bit-identical);
 *  - the queries' checks and codes apply: heat-map mode is RTX_ERR_STATE, any other flag RTX_ERR_INVALID_ARG, and so is RTX_QUERY_SORT
 *    (the hooks answer in the caller's order);
 *  - any n >= 1 (rounds of RTX_QUERY_CHUNK_RAYS; the earlier limit of 4096 tiles of 1024 rays is gone); the frame's queues, a queued frame and what rtx_get_stats has yet to read are untouched.
 * Still RTX_ERR_INVALID_ARG: rtx_debug_trace_rays on a context with bounces < 1, rtx_debug_occluded on a frame without lights. */
int rtx_debug_trace_rays(rtx_ctx * ctx, const float * rays18, int32_t n, float * hits27, uint32_t flags);
/* Scene::intersect_primitives (Scene.cpp:182-190) of n segments (7 floats: origin, direction, max distance) in host memory through the
 * production shadow-ray kernel: occluded[i] = 1 / 0.  See rtx_debug_trace_rays. */
int rtx_debug_occluded(rtx_ctx * ctx, const float * origin_direction_maxdist7, int32_t n, uint32_t * occluded, uint32_t flags);
/* Point / Spot / DirectionalLight::calc_lighting (10 floats in: normal, to_light, to_camera, distance^2; 9 out) and Window::plot */
int rtx_debug_light_plot(rtx_ctx * ctx, const rtx_point_light * pl, const rtx_spot_light * sl, const rtx_directional_light * dl,
                         const float * in10, float * out9, int32_t n_light, const float * rgb, uint32_t * packed, int32_t n_plot);
/* the group path of `world` ranks replayed on this one GPU without RCCL (partition, tile-major writes, frame assembly) */
int rtx_debug_group_loopback(rtx_ctx * ctx, int32_t world, uint32_t flags);
/* the shadow-ray packet walk of an uploaded mesh: *stack_need = packet-stack entries its 4-wide records can need, or -1 when the mesh keeps
 * the binary walk (boxes not nested / limits exceeded) */
int rtx_debug_blas_wide(rtx_ctx * ctx, int32_t blas_id, int32_t * stack_need);
/* the per-lane part of the closest-hit packet walk of an uploaded mesh: *stack_need = stack entries a lane's walk of the ordered 4-wide records
 * can need, or -1 when the mesh keeps the binary walk (boxes not nested / a leaf of 16+ triangles / 2^24+ nodes or triangles) */
int rtx_debug_blas_wide_closest(rtx_ctx * ctx, int32_t blas_id, int32_t * stack_need);
/* the node layouts derived from the lane layout, as the kernels read them now, to host (beside rtx_read_blas / rtx_read_frame_state: waits
 * for the stream, plain device-to-host copies, launches nothing, changes nothing).  info8[0] = node slots n, [1] / [2] = 1 when the mesh has the
 * shadow-ray / the closest-hit 4-wide records, [3..5] = floats in the x / y / z plane list, [6..7] = 0.  pk_nodes: n x 8 floats (min.x, min.y,
 * max.x, max.y, min.z, max.z, left_or_first, count); pk4_nodes, pk4c_nodes: (2n + 4) record slots x 8 floats (the same box order, first,
 * leaf count / meta), left alone when the mesh has none; planes_*: the sorted plane lists.  Any pointer may be NULL (call once with the arrays
 * NULL to learn the sizes).  blas_id -1: the TLAS of the current frame: info8[0] = its node slots, pk_nodes its packet layout, no other array
 * is written.  RTX_ERR_INVALID_ARG: an id below -1 or above the id range; RTX_ERR_STATE: no BLAS uploaded under that id / before rtx_set_frame. */
int rtx_debug_read_layouts(rtx_ctx * ctx, int32_t blas_id, int32_t * info8, float * pk_nodes, float * pk4_nodes, float * pk4c_nodes,
                           float * planes_x, float * planes_y, float * planes_z);
/* the grids the context launches, as rtx_create sized them from the device, RTX_GRID_CUS and the grid knobs (launches nothing): out[0] = compute
 * units the grids are sized for, [1..3] = workgroups of the per-lane closest-hit, the per-lane shadow-ray and the plain traversal launches
 * (256 threads each), [4..5] = workgroups of the closest-hit and the shadow-ray packet launches (one wave each), [6] = workgroups of the item
 * launch (one wave each), [7] = threads the per-thread spill regions hold */
int rtx_debug_grids(rtx_ctx * ctx, int32_t out[8]);
/* Sky::sample (Sky.cpp:28-68) of the uploaded sky at n directions */
int rtx_debug_sky_sample(rtx_ctx * ctx, const float * directions_xyz, float * out_rgb, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* RTX_H */
