// rtx_api.hip — host side of librtx_hip.so: the C ABI of include/rtx.h over the gfx950 kernels.
//
// One context = one GPU, one HIP stream.  Scene data is uploaded once and stays resident in HBM;
// rtx_set_frame uploads what Scene::update produces (< 8 KiB for 16 instances); rtx_render_tiles
// enqueues the whole wavefront pipeline for a batch of tiles without any host synchronisation:
//
//   for level = 0 .. bounces:  k_trace<closest>  ->  k_shade  ->  k_trace<any>
//   for level = bounces .. 0:  k_resolve
//
// Queue sizes are only known on the device (DevCounters), so every kernel reads its element count
// from HBM and the launch geometry is fixed (persistent grids).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <string>
#include <vector>
#include <algorithm>
#include <type_traits>

#include "../../include/rtx.h"
#include "rtx_device.h"
#include "rtx_math.h"
#include "rtx_libm.h"
#include "rtx_texture.h"
#include "rtx_trace.h"
#include "rtx_shade.h"
#include "rtx_packet.h"
#include "rtx_present.h"
#include "rtx_update.h"
#include "rtx_refit.h"
#include "rtx_build.h"
#include "rtx_normals.h"
#include "rtx_query.h"
#include "rtx_nearest.h"
#include "rtx_hits.h"
#include "rtx_sweep.h"
#include "rtx_overlap.h"
#include "rtx_capsule.h"
#include "rtx_boxsweep.h"
#include "rtx_texmip.h"
#include <rocprim/device/device_radix_sort.hpp>      // rtx_update_instances, scenes beyond one workgroup: header-only, part of ROCm
#include "rtx_hostmem.h"                             // DevBuf, StageRing, grow_keep: every device and pinned allocation has one owner
#include "rtx_layout_host.h"                         // convert_nodes*, build_nodes_pk4*, parent_table, balanced_topology: trees to the layouts of rtx_layout.h (no HIP in it; layout_check.cpp)
#include "rtx_plan.h"                                // Knobs, plan_render: which kernels a render call launches (no HIP in it; plan_check.cpp)

#define SLOT_BUDGET (48ll * 1000 * 1000)      // ray slots per batch of tiles (see plan_batch)

// Tuning knobs (struct Knobs, rtx_plan.h): read here, once per context in rtx_create
static long long knob_int(const char * name, long long dflt, long long lo, long long hi) {
    const char * e = getenv(name);
    if (!e || !*e) return dflt;
    char * end = nullptr; const long long v = strtoll(e, &end, 10);
    if (end == e || *end != 0 || v < lo || v > hi) { fprintf(stderr, "librtx_hip: %s=%s ignored (expected an integer in [%lld, %lld])\n", name, e, lo, hi); return dflt; }
    return v;
}
static double knob_real(const char * name, double dflt, double lo, double hi) {
    const char * e = getenv(name);
    if (!e || !*e) return dflt;
    char * end = nullptr; const double v = strtod(e, &end);
    if (end == e || *end != 0 || !(v >= lo && v <= hi)) { fprintf(stderr, "librtx_hip: %s=%s ignored (expected a number in [%g, %g])\n", name, e, lo, hi); return dflt; }
    return v;
}
struct KernelTime { const char * name; hipEvent_t a, b; };

struct rtx_ctx {
    rtx_config cfg;
    hipStream_t stream = nullptr;        // stream all work is enqueued on
    hipStream_t own_stream = nullptr;    // created by rtx_create
    hipStream_t any_stream = nullptr;    // shadow-ray kernels run here, overlapping the next levels' closest-hit / shade kernels
    hipEvent_t ev_shade0 = nullptr, ev_shade_last = nullptr, ev_any_done = nullptr;
    void * ext_rgb = nullptr, * ext_packed = nullptr;
    std::string err;
    int n_cu = 0;

    // Every device and pinned allocation below belongs to a DevBuf or a StageRing member (rtx_hostmem.h) and dies with the context: there is no
    // list of buffers to keep anywhere.  Per BLAS id: h_blas[id] is the id's entry of the contiguous table the kernels read (uploaded to d_blas),
    // blas[id] the host's record of it; both vectors are resized together (commit_blas).
    // rtx_bind_blas_vertices / rtx_refit_blas: the record-slot -> node maps of the 4-wide layouts as the upload laid them out (empty: binary
    // walk), and once bound the plan's device block and the kernel arguments of a refit, which point into it
    struct BlasRefit { std::vector<int32_t> map4, map4c; bool bound = false; int32_t vertex_count = 0; DevBuf block; DevRefit dev; float * planes[3] = { nullptr, nullptr, nullptr }; void * sort_tmp = nullptr; size_t sort_bytes = 0; };
    // rtx_alloc_blas / rtx_build_blas: the scratch block and the kernel arguments of a build
    struct BlasBuild { bool allocated = false; DevBuf block; DevBuild dev; void * sort_tmp = nullptr; size_t sort_bytes = 0; int levels = 0; };
    // max_local_material, inner_depth: for validate_references(), which checks every id a kernel will follow on the host before anything is
    // launched; packet_ok: the tree fits the packet kernels' packed entries (plan_stack_limits)
    // rtx_alloc_blas_topology / rtx_set_blas_topology / rtx_blas_vertex_normals: the block of the vertex normals' buffers and the kernel
    // arguments that point into it; set: a topology has been queued since the alloc
    struct BlasNormals { bool allocated = false, set = false; DevBuf block; DevNormals dev; void * sort_tmp = nullptr; size_t sort_bytes = 0; unsigned int key_bits = 0; };
    // rtx_blas_pseudonormals: the block of the pseudonormal tables (face records, vert_pn, edge_pn) and the kernel arguments that point into
    // it and into the topology's and the refit plan's blocks; made by the first call for an id
    struct BlasSide { bool allocated = false; DevBuf block; DevSide dev; };
    struct BlasHost { std::vector<DevBuf> arrays; int max_local_material = -1, inner_depth = -1; bool packet_ok = true; BlasRefit refit; BlasBuild build; BlasNormals normals; BlasSide side; };
    std::vector<DevBlas> h_blas;
    std::vector<BlasHost> blas;
    DevBuf d_blas, d_materials, d_textures, d_sky, d_ewa;
    std::vector<DevTexture> h_tex;
    std::vector<DevBuf> tex_texels;             // per texture id, beside h_tex
    // rtx_alloc_texture / rtx_update_texture: per texture id, beside h_tex — allocated: the chain is this project's own (rtx_upload_texture
    // clears it), plan: the launches of an update, made once at the alloc; the byte -> linear table of RTX_TEXELS_RGBA8_SRGB, once per context
    struct TexUpdate { bool allocated = false; rtxt::Plan plan; };
    std::vector<TexUpdate> tex_update;
    DevBuf d_srgb_lut;
    bool sky_uploaded = false;                  // rtx_update_sky copies over the probe rtx_upload_sky made, not over the context's black default
    int material_count = 0, sky_size = 0;
    std::vector<rtx_material> h_materials; int tlas_inner_depth = -1; std::vector<int> frame_primitive_materials; bool refs_dirty = true; Knobs knobs; int item_blocks = 0, item_cap_alloc = 0; DevBuf d_pk_items, d_pk_item_count;

    // per-frame state (rtx_set_frame): ONE device block, filled by one asynchronous copy on the context's stream from a ring of pinned
    // staging buffers (stage_copy) — the host never waits for the GPU between frames (cfg5: Scene::update + TLAS rebuild every frame)
    DevBuf d_frame;
    StageRing frame_ring;
    DevScene scene;
    bool frame_set = false;
    // every instance of the frame is a rigid pose (rtxu::instance_rigid): judged from the matrices rtx_set_frame is handed, true after
    // rtx_update_instances by its unit-quaternion contract; the length queries refuse a frame that is not (walk_setup)
    bool frame_rigid = true;
    // plan_lone_facts of the state rtx_set_frame was handed; rtx_update_instances clears both (poses and TLAS made on the device: the host has not
    // seen the matrices).  DevScene::lone / copy_class are these with the knob applied
    LoneFacts frame_lone = { false, false };
    // rtx_update_instances: a device block of its own for the updated instances / TLAS (both node layouts) / indices and the builder's scratch
    // (AABBs, bounds, keys), grown only; the DevScene pointers are switched to it, the rest of the frame stays in d_frame.  d_upd_sort = rocPRIM's
    // temporary storage and the unsorted keys (multi-launch path), grown only
    DevBuf d_upd, d_upd_sort; int upd_cap = 0;
    // rtx_set_views: the cameras of a batch of views (device array, grown only, filled through a staging ring of its own like the frame block)
    // and the view framebuffer (vfb_cap views, allocated on first use, grown only) or the caller's buffers of ext_vcap views
    // (rtx_bind_view_framebuffer)
    DevBuf d_views, d_vfb_rgb, d_vfb_packed;
    StageRing view_ring;
    int32_t view_count = 0, vfb_cap = 0, ext_vcap = 0;
    void * ext_vrgb = nullptr, * ext_vpacked = nullptr;
    // ray views (rtx_set_rays / rtx_bind_rays): the context's own ray buffer of ray_count views (grown only, filled through a staging ring of
    // its own like the cameras) or the caller's device buffer of ext_ray_count views; independent of the rtx_set_views state
    DevBuf d_rays;
    StageRing ray_ring;
    int32_t ray_count = 0, ext_ray_count = 0;
    const void * ext_rays = nullptr;
    // rtx_bind_aovs: the bound channels (RTX_AOV_* bits) and where they go: the caller's device buffers of aov_ext_cap pixels (aov_ext), or
    // the context's own buffers d_aov[k] of aov_own_cap[k] pixels (allocated by the first call that writes the channel, grown only)
    uint32_t aov_channels = 0; bool aov_ext = false; int64_t aov_ext_cap = 0; DevAov aov_ext_ptrs = {};
    DevBuf d_aov[8]; int64_t aov_own_cap[8] = {};

    DevQueues q;
    DevBuf qb[20];
    // rtx_query_closest / rtx_query_occluded: a queue set of their own (query_queues), one chunk of query_cap slots, grown only; counters and
    // packet-queue heads of their own too, so a query never resets what rtx_get_stats has yet to read of a render call
    DevBuf d_query[4], d_query_counters, d_query_heads; int32_t query_cap = 0;
    // RTX_QUERY_SORT: unsorted and sorted keys, the twelve bounds and rocPRIM's temporary storage, for query_sort_cap slots; nothing until the first sorted call
    DevBuf d_query_sort; int32_t query_sort_cap = 0; size_t query_sort_tmp = 0;
    // rtx_query_nearest: the tile counter of a round (4 bytes, made by the first call); RTX_NEAREST_FETCH=0: tiles by stride, no counter (A/B)
    DevBuf d_nearest_head; bool nearest_fetch = true;
    // rtx_query_nearest / rtx_query_hits / rtx_query_sweep / rtx_query_overlap / rtx_query_sweep_box: RTX_QUERY_GRID=g caps their grids at g workgroups (0: the spill region's size alone decides)
    int query_grid = 0;
    // rtx_set_object_masks / rtx_update_object_masks: the table the filtered walk queries read (M uint32_t, grown only, filled through a staging
    // ring of its own like the cameras), whether there is one, and (I, S, P) of the frame it was set for
    DevBuf d_object_masks; StageRing mask_ring; bool masks_set = false; int32_t mask_counts[3] = { 0, 0, 0 };
    // rtx_query_signed_distance: one DevSideBlas per BLAS id (all null: no tables), beside h_blas / d_blas and not in them, so DevBlas and the
    // render kernels are what they were.  h_side follows the ids' states (rtx_blas_pseudonormals sets an entry, commit_blas and a replaced
    // topology clear it); the device copy is brought up to date by the next signed query, on the stream, through a staging ring of its own
    std::vector<DevSideBlas> h_side; DevBuf d_side; StageRing side_ring; bool side_dirty = true;
    size_t slots_alloc = 0, shadow_alloc = 0;
    DevBuf d_stats_partial, d_pk_fifo, d_counters, d_spill, d_fb_rgb, d_fb_packed, d_display, d_gamma, d_pk_heads;
    int trace_blocks_closest = 0, trace_blocks_any = 0, trace_blocks_count = 0;
    int pk_blocks_closest = 0, pk_blocks_any = 0;    // persistent grids of the packet kernels (even: waves % 8 == 0, see k_begin_batch)

    rtx_stats stats_acc; rtx_work_counters work_acc; uint32_t err_flags_acc = 0;
    bool stats_pending = false;

    bool timing = false;
    bool serial = false;                 // RTX_RENDER_SERIAL: keep every kernel on one stream (per-kernel timings without overlap)
    // RTX_GRAPH=1: the launches of a rtx_render_tiles call are captured once into a hipGraph and replayed while nothing they depend on changes
    hipGraphExec_t graph_exec = nullptr; std::vector<unsigned char> graph_key, graph_warm;
    // RTX_PK_LPT: level-0 closest-hit packets longest first, by their cost in the previous call with the same tiles (k_packet_order on a side stream)
    DevBuf d_pk_cost, d_pk_order; hipStream_t order_stream = nullptr; hipEvent_t ev_cost = nullptr, ev_order = nullptr; int32_t lpt_key[5] = { -1, -1, -1, -1, -1 }; bool lpt_valid = false;
    std::vector<KernelTime> times;
    std::vector<hipEvent_t> event_pool;
    size_t event_next = 0;
};

extern "C" int rtx_abi_version(void) { return RTX_ABI_VERSION; }

extern "C" const char * rtx_last_error(const rtx_ctx * ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" int rtx_create(const rtx_config * config, rtx_ctx ** out_ctx) {
    if (!config || !out_ctx) return RTX_ERR_INVALID_ARG;
    *out_ctx = nullptr;
    if (config->width <= 0 || config->height <= 0 || config->bounces < 0) return RTX_ERR_INVALID_ARG;
    if (config->bounces + 1 > RTX_MAX_LEVELS) return RTX_ERR_LIMIT;
    if (config->stack_size < 1 || config->stack_size > RTX_MAX_STACK) return RTX_ERR_LIMIT;
    if (config->traversal_strategy < 0 || config->traversal_strategy > 1 || config->texture_mode < 0 || config->texture_mode > 2 ||
        config->mip_filter < 0 || config->mip_filter > 2) return RTX_ERR_INVALID_ARG;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return RTX_ERR_NO_DEVICE;
    if (config->device < 0 || config->device >= n_dev) return RTX_ERR_NO_DEVICE;
    if (hipSetDevice(config->device) != hipSuccess) return RTX_ERR_NO_DEVICE;

    rtx_ctx * c = new rtx_ctx();
    c->cfg = *config;
    memset(&c->scene, 0, sizeof(c->scene));
    memset(&c->q, 0, sizeof(c->q));
    memset(&c->stats_acc, 0, sizeof(c->stats_acc));
    memset(&c->work_acc, 0, sizeof(c->work_acc));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, config->device) != hipSuccess) { delete c; return RTX_ERR_HIP; }
    c->n_cu = prop.multiProcessorCount;
    {   // RTX_GRID_CUS=n (tests, A/B runs): every grid below is sized as if the device had n compute units, 1 .. the device's count (more: the
        // device's count).  The persistent kernels then go through their dynamic rounds on frames of a few tiles (tests/test_gpu_small_grids.py)
        const long long cus = knob_int("RTX_GRID_CUS", c->n_cu, 1, 1 << 20);
        if (cus < c->n_cu) c->n_cu = (int)cus;
    }
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) { delete c; return RTX_ERR_HIP; }
    c->stream = c->own_stream;
    // any_stream is created on first use (two-stream mode only): HIP multiplexes streams onto a few hardware queues, and an unused
    // stream per context would push other contexts' streams onto shared queues
    hipEventCreateWithFlags(&c->ev_shade0, hipEventDisableTiming); hipEventCreateWithFlags(&c->ev_shade_last, hipEventDisableTiming);
    hipEventCreateWithFlags(&c->ev_any_done, hipEventDisableTiming);

    // Texture::init(alpha = 2) EWA weight table, Texture.h:53-62 (host libm, like the reference; shipped as data)
    float ewa[RTX_EWA_LUT_SIZE];
    {
        const float alpha = 2.0f;
        const float denom = 1.0f / (float)(RTX_EWA_LUT_SIZE - 1);
        const float exp_neg_alpha = expf(-alpha);
        for (int i = 0; i < RTX_EWA_LUT_SIZE; i++) { float r2 = (float)i * denom; ewa[i] = expf(-alpha * r2) - exp_neg_alpha; }
    }
    int rc = upload(c, c->d_ewa, ewa, sizeof(ewa));
    // MaterialBuffer::init(): material 0 = black default, Material.h:52-60
    rtx_material m0; memset(&m0, 0, sizeof(m0)); m0.texture_id = -1; m0.index_of_refraction = 1.0f;
    if (!rc) rc = upload(c, c->d_materials, &m0, sizeof(m0));
    c->material_count = 1;
    // Window framebuffer, Window.cpp:42,76
    const size_t px = (size_t)config->width * config->height;
    if (!rc) rc = ensure(c, c->d_fb_rgb, px * 12);
    if (!rc) rc = ensure(c, c->d_fb_packed, px * 4);
    if (!rc) rc = ensure(c, c->d_counters, sizeof(DevCounters));
    if (!rc) rc = ensure(c, c->d_pk_heads, (size_t)2 * (RTX_MAX_LEVELS + 1) * RTX_PK_CLASSES * 32 * sizeof(uint32_t));
    float zero_sky[6] = { 0, 0, 0, 0, 0, 0 };
    if (!rc) rc = upload(c, c->d_sky, zero_sky, sizeof(zero_sky));
    c->sky_size = 1;
    if (rc) { rtx_destroy(c); return rc; }
    hipMemset(c->d_fb_rgb.p, 0, px * 12);
    hipMemset(c->d_fb_packed.p, 0, px * 4);

    // ---- knobs: parsed once, validated, clamped (see struct Knobs) ----
    Knobs & K = c->knobs;
    K.slot_budget = knob_int("RTX_SLOT_BUDGET", SLOT_BUDGET, 1024, 1ll << 31);
    K.item_bytes_max = knob_int("RTX_PK_ITEM_BYTES", 1ll << 30, 0, 1ll << 36);
    K.shade_grid = (int)knob_int("RTX_SHADE_GRID", 4, 1, 64);
    K.lane_from_level = (int)knob_int("RTX_LANE_FROM_LEVEL", -1, 0, 1 << 20);
    K.lane_from_level_any = (int)knob_int("RTX_LANE_FROM_LEVEL_ANY", -1, 0, 1 << 20);
    K.split_items = (int)knob_int("RTX_PK_SPLIT", 256, 0, 1 << 16);
    if (K.split_items > 0) K.split_items = (K.split_items + 63) & ~63;          // chunks are whole units of 64 items
    K.resolve_block = (int)knob_int("RTX_RESOLVE_BLOCK", 256, 64, 256);
    if (K.resolve_block != 64 && K.resolve_block != 128 && K.resolve_block != 256) K.resolve_block = 256;
    K.pk4_order = (int)knob_int("RTX_PK4_ORDER", 1, 0, 1);
    K.merge_any = knob_int("RTX_SERIAL_MERGE_ANY", 1, 0, 1) != 0;       // one-stream mode: ONE shadow-ray launch for all levels after the last shade (0: one per level)
    K.no_wide = knob_int("RTX_PK_WIDE", 1, 0, 1) == 0;                  // 0: binary shadow-ray walk for every mesh
    K.lpt = (int)knob_int("RTX_PK_LPT", -1, -1, 1);                     // level-0 closest-hit packets longest first (last frame's cost): 1 always, 0 never, -1: in the two-stream (one frame at a time) shape
    K.graph = knob_int("RTX_GRAPH", 0, 0, 1) != 0;                      // 1: identical rtx_render_tiles calls replay a captured hipGraph
    K.no_wide_closest = knob_int("RTX_PK_WIDE_CLOSEST", 1, 0, 1) == 0;  // 0: binary per-lane phase of the closest-hit walk for every mesh
    K.fuse_shade = knob_int("RTX_FUSE_SHADE", 0, 0, 1) != 0;      // measured: 1.51 vs 1.28 ms per cfg3 frame with three frames in flight: off
    K.update_small_max = (int)knob_int("RTX_UPDATE_SMALL_MAX", RTX_UPDATE_SMALL_MAX, 0, RTX_UPDATE_SMALL_MAX);
    K.tex_pass_levels = (int)knob_int("RTX_TEX_PASS_LEVELS", rtxt::DEFAULT_PASS_LEVELS, 1, rtxt::MAX_PASS_LEVELS);      // DESIGN.md 9, Device-side texture update
    c->nearest_fetch = knob_int("RTX_NEAREST_FETCH", 1, 0, 1) != 0;     // rtx_query_nearest: workgroups fetch tiles from a counter (1) or take them by stride (0): DESIGN.md 9
    c->query_grid = (int)knob_int("RTX_QUERY_GRID", 0, 0, 1 << 20);    // the walk queries: at most this many workgroups, each takes tile after tile (0: no cap); tests/test_gpu_query_tiles.py
    K.lone_entry = knob_int("RTX_PK_LONE_ENTRY", 1, 0, 1) != 0;         // 0: the packet kernels take the TLAS iterator path for every scene (A/B runs, tests/test_gpu_lone_entry.py)
    K.fail_item_alloc = knob_int("RTX_DEBUG_FAIL_ITEM_ALLOC", 0, 0, 1) != 0;      // tests: the item buffer's allocation fails (a size no device has), the fallback kernel must take over
    int bpc = 0;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, k_trace_fast<false>, RTX_TRACE_BLOCK, 0);
    c->trace_blocks_closest = c->n_cu * (bpc > 0 ? bpc : 2);
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, k_trace_fast<true>, RTX_TRACE_BLOCK, 0);
    c->trace_blocks_any = c->n_cu * (bpc > 0 ? bpc : 2);
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, k_trace<false, true>, RTX_TRACE_BLOCK, 0);
    c->trace_blocks_count = c->n_cu * (bpc > 0 ? bpc : 2);
    if (K.fuse_shade) hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, k_packet<false, false, false, true, false>, RTX_PK_BLOCK, 0);      // one grid size for every closest-hit packet launch of a context
    else              hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, k_packet<false, false>, RTX_PK_BLOCK, 0);
    c->pk_blocks_closest = (c->n_cu * (bpc > 0 ? bpc : 4) + 1) & ~1;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, k_packet<true, false>, RTX_PK_BLOCK, 0);
    c->pk_blocks_any = (c->n_cu * (bpc > 0 ? bpc : 4) + 1) & ~1;
    {   // persistent-grid sizes of the packet kernels (A/B runs): a scale on the occupancy-derived size, or blocks per CU
        const double f = knob_real("RTX_PK_GRID_SCALE", 1.0, 0.05, 16.0);
        if (f != 1.0) { c->pk_blocks_closest = ((int)(c->pk_blocks_closest * f) + 1) & ~1; c->pk_blocks_any = ((int)(c->pk_blocks_any * f) + 1) & ~1; }
        const double fa = knob_real("RTX_PK_GRID_ANY", 0.0, 0.05, 64.0), fc = knob_real("RTX_PK_GRID_CLOSEST", 0.0, 0.05, 64.0);
        if (fa > 0.0) c->pk_blocks_any = ((int)(c->n_cu * fa) + 1) & ~1;
        if (fc > 0.0) c->pk_blocks_closest = ((int)(c->n_cu * fc) + 1) & ~1;
    }
    {   // the packet queues hand out packets k * 8 + head after a static first round of one packet per wave: whole rounds only, so waves % 8 == 0
        const int g = RTX_PK_CLASSES * RTX_WAVE / RTX_PK_BLOCK > 1 ? RTX_PK_CLASSES * RTX_WAVE / RTX_PK_BLOCK : 1;
        c->pk_blocks_any = (c->pk_blocks_any + g - 1) / g * g; c->pk_blocks_closest = (c->pk_blocks_closest + g - 1) / g * g;
        if (c->pk_blocks_any < g) c->pk_blocks_any = g;      // a fraction of very few compute units (RTX_PK_GRID_* with RTX_GRID_CUS) rounds to no workgroup at all
        if (c->pk_blocks_closest < g) c->pk_blocks_closest = g;
    }
    // threads of the largest launch that indexes the per-thread spill / work-list regions with its global thread id
    long long max_threads = (long long)(c->trace_blocks_closest > c->trace_blocks_any ? c->trace_blocks_closest : c->trace_blocks_any) * RTX_TRACE_BLOCK;
    if ((long long)c->trace_blocks_count * RTX_TRACE_BLOCK > max_threads) max_threads = (long long)c->trace_blocks_count * RTX_TRACE_BLOCK;
    if ((long long)c->pk_blocks_any * RTX_PK_BLOCK > max_threads) max_threads = (long long)c->pk_blocks_any * RTX_PK_BLOCK;       // the packet kernels' per-lane phases spill there too
    if ((long long)c->pk_blocks_closest * RTX_PK_BLOCK > max_threads) max_threads = (long long)c->pk_blocks_closest * RTX_PK_BLOCK;
    // deferral thresholds of the hybrid walks are lane counts (0 .. 64), the growth a shift count: anything else would reach the asm walkers as garbage
    c->q.pk_defer_t0 = (int)knob_int("RTX_PK_DEFER", 8, 0, 64);
    c->q.pk_defer_leaf = (int)knob_int("RTX_PK_DEFER_LEAF", c->q.pk_defer_t0 / 2, 0, 64);
    c->q.pk_defer_t0_closest = (int)knob_int("RTX_PK_DEFER_CLOSEST", 64, 0, 64);
    c->q.pk_closest_asm = (int)knob_int("RTX_PK_CLOSEST_ASM", 1, 0, 1);
    c->q.pk_defer_t0_primary = (int)knob_int("RTX_PK_DEFER_PRIMARY", c->q.pk_closest_asm ? 4 : 64, 0, 64);
    c->q.pk_order = (int)knob_int("RTX_PK_ORDER", 1, 0, 1);
    c->q.prof_level = (int)knob_int("RTX_LANE_PROF_LEVEL", 2, 0, 100 + RTX_MAX_LEVELS);      // -DRTX_LANE_PROF builds only (tools/lane_prof.py)
    c->q.pk_defer_grow = (int)knob_int("RTX_PK_GROW", 3, 0, 31);
    c->q.spill_threads = (int)max_threads;
    rc = ensure(c, c->d_spill, (size_t)c->q.spill_threads * (RTX_MAX_STACK - RTX_LDS_STACK) * 4 * 3);   // three regions, see k_trace_fast
    if (!rc) rc = ensure(c, c->d_pk_fifo, (size_t)c->q.spill_threads * RTX_PK_FIFO * 8);        // (reference, key) per work-list entry
    { int ib = 0; hipOccupancyMaxActiveBlocksPerMultiprocessor(&ib, k_items, RTX_ITEM_BLOCK, 0); c->item_blocks = c->n_cu * (ib > 0 ? ib : 4);
      const double f = knob_real("RTX_ITEM_GRID", 0.0, 0.05, 64.0); if (f > 0.0) c->item_blocks = (int)(c->n_cu * f) > 0 ? (int)(c->n_cu * f) : 1; }
    c->q.pk_items = nullptr; c->q.pk_item_count = nullptr; c->q.pk_item_cap = 0;      // sized per render call (render_tiles_impl)
    if (rc) { rtx_destroy(c); return rc; }
    bind_tables(c);                      // the default material and sky; from here on every change of a table rebinds (replace_table)
    *out_ctx = c;
    return RTX_OK;
}

extern "C" int rtx_destroy(rtx_ctx * c) {
    if (!c) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->event_pool) hipEventDestroy(e);
    if (c->graph_exec) { hipGraphExecDestroy(c->graph_exec); c->graph_exec = nullptr; }
    if (c->order_stream) { hipStreamSynchronize(c->order_stream); hipStreamDestroy(c->order_stream); hipEventDestroy(c->ev_cost); hipEventDestroy(c->ev_order); }
    if (c->any_stream) { hipStreamSynchronize(c->any_stream); hipStreamDestroy(c->any_stream); }
    if (c->ev_shade0) hipEventDestroy(c->ev_shade0);
    if (c->ev_shade_last) hipEventDestroy(c->ev_shade_last);
    if (c->ev_any_done) hipEventDestroy(c->ev_any_done);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;                            // the device is current: every DevBuf and StageRing of the context releases its memory here
    return RTX_OK;
}

// Walks the nodes a traversal can reach from the root (abandoned child pairs and index 1 hold garbage in reference-built arrays and are
// not looked at): every leaf range inside the primitive array, every child pair inside the node array, and no node reachable twice —
// a cycle would keep a GPU traversal going for ever.
static bool validate_tree(const rtx_bvh_node * nodes, int node_count, int64_t primitive_count, int * max_inner_depth = nullptr, int * max_leaf_count = nullptr) {
    if (node_count < 1) return false;
    std::vector<unsigned char> seen((size_t)node_count, 0);
    std::vector<std::pair<int, int>> stack(1, std::make_pair(0, 0));       // node, depth
    int deepest = -1, biggest = 0;
    while (!stack.empty()) {
        const int i = stack.back().first, d = stack.back().second; stack.pop_back();
        if (seen[i]) return false;
        seen[i] = 1;
        const int cnt = nodes[i].count & 0x3fffffff, f = nodes[i].left_or_first;
        if (cnt > 0) { if (f < 0 || (int64_t)f + cnt > primitive_count) return false; if (cnt > biggest) biggest = cnt; }
        else { if (f < 0 || f + 1 >= node_count) return false; if (d > deepest) deepest = d; stack.push_back(std::make_pair(f, d + 1)); stack.push_back(std::make_pair(f + 1, d + 1)); }
    }
    if (max_inner_depth) *max_inner_depth = deepest;
    if (max_leaf_count) *max_leaf_count = biggest;
    return true;
}


// ---- BLAS upload: stage, then commit -----------------------------------------------------------------------------------------------
// Everything an id will hold is built into a BlasStaged first, which owns its allocations; commit_blas swaps it in.  A call that is refused
// or fails on the way therefore leaves the id as it was (or empty), and what it had allocated dies with the staged record.
struct BlasStaged { DevBlas B; rtx_ctx::BlasHost H; };

// one more device array of a staged mesh: `bytes` allocated, the first `copy` filled from src
template <typename T> static int stage_array(rtx_ctx * c, std::vector<DevBuf> & arrays, const void * src, size_t copy, size_t bytes, const T ** out) {
    DevBuf b;
    if (int rc = ensure(c, b, bytes)) return rc;
    if (copy) HIP_OK(c, hipMemcpy(b.p, src, copy, hipMemcpyHostToDevice));
    *out = (const T *)b.p;
    arrays.push_back(std::move(b));
    return RTX_OK;
}

// the device table and h_blas become `table` (replace_table: a table that has to grow is built beside the old one, which a failure leaves in
// place, and the scene is bound to what the context then holds); accept() is the rest of the host state that changes with it
template <typename Accept> static int upload_blas_table(rtx_ctx * c, std::vector<DevBlas> & table, Accept && accept) {
    return replace_table(c, c->d_blas, table.data(), table.size() * sizeof(DevBlas), [&] { c->h_blas.swap(table); accept(); });
}

// the id has no pseudonormal tables (any more): the next signed query uploads the entry before it launches, and none is queued now — every
// caller has waited for the stream
static void drop_side_entry(rtx_ctx * c, int32_t blas_id) {
    if ((size_t)blas_id < c->h_side.size() && c->h_side[blas_id].vert_pn) { memset(&c->h_side[blas_id], 0, sizeof(DevSideBlas)); c->side_dirty = true; }
}

// The one place an id's state changes hands.  Queued work may still read the old arrays and the table: it is waited for explicitly, then the
// table is uploaded with the new entry (replace_table does both), and only then does the old record — arrays, refit plan, build scratch — go.
static int commit_blas(rtx_ctx * c, int32_t blas_id, BlasStaged & S) {
    std::vector<DevBlas> table = c->h_blas;
    if ((size_t)blas_id >= table.size()) { DevBlas none; memset(&none, 0, sizeof(none)); table.resize(blas_id + 1, none); }
    table[blas_id] = S.B;
    return upload_blas_table(c, table, [&] {
        if (c->blas.size() < c->h_blas.size()) c->blas.resize(c->h_blas.size());
        c->blas[blas_id] = std::move(S.H);
        c->refs_dirty = true;
        drop_side_entry(c, blas_id);                                // the pseudonormal tables went with the old record
    });
}

// All checks, then all allocations and copies, into S; the context is only read.
// pk4_order: the slot order of the 4-wide shadow-ray records (build_nodes_pk4): the context's knob for rtx_upload_blas, 0 for rtx_alloc_blas
static int stage_blas(rtx_ctx * c, int32_t blas_id, const rtx_bvh_node * nodes, int32_t node_count,
                      const rtx_triangle_hot * tri_hot, const rtx_triangle_cold * tri_cold,
                      int32_t triangle_count, int32_t material_offset, int pk4_order, BlasStaged & S) {
    if (!c || blas_id < 0 || blas_id >= (1 << 20) || !nodes || node_count <= 0 || triangle_count < 0 || (triangle_count > 0 && (!tri_hot || !tri_cold)))
        return RTX_ERR_INVALID_ARG;
    // every leaf must address triangles inside the arrays, every inner node children inside the node array
    int inner_depth = -1, leaf_max = 0;
    if (!validate_tree(nodes, node_count, triangle_count, &inner_depth, &leaf_max)) return RTX_ERR_INVALID_ARG;
    int max_local = -1;
    for (int i = 0; i < triangle_count; i++) { if (tri_cold[i].material_id < 0) return RTX_ERR_INVALID_ARG; if (tri_cold[i].material_id > max_local) max_local = tri_cold[i].material_id; }
    hipSetDevice(c->cfg.device);

    std::vector<float4> nd; convert_nodes(nodes, node_count, nd);
    std::vector<float4> th((size_t)RTX_TRI_STRIDE * (triangle_count > 0 ? triangle_count : 1), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (int i = 0; i < triangle_count; i++) {
        th[RTX_TRI_STRIDE * (size_t)i]     = make_float4(tri_hot[i].position_0[0], tri_hot[i].position_0[1], tri_hot[i].position_0[2], 0.0f);
        th[RTX_TRI_STRIDE * (size_t)i + 1] = make_float4(tri_hot[i].position_edge_1[0], tri_hot[i].position_edge_1[1], tri_hot[i].position_edge_1[2], 0.0f);
        th[RTX_TRI_STRIDE * (size_t)i + 2] = make_float4(tri_hot[i].position_edge_2[0], tri_hot[i].position_edge_2[1], tri_hot[i].position_edge_2[2], 0.0f);
    }
    std::vector<float4> ndp; convert_nodes_pk(nodes, node_count, ndp);
    rtx_ctx::BlasHost & H = S.H;
    std::vector<float4> nd4; int need4 = 0;
    const bool wide = !c->knobs.no_wide && build_nodes_pk4(nodes, node_count, triangle_count, nd4, &need4, pk4_order, RTX_PK4_MAX_NEED, &H.refit.map4) && need4 <= RTX_PK4_MAX_NEED;
    std::vector<float4> nd4c; int need4c = 0;
    const bool wide_closest = !c->knobs.no_wide_closest && build_nodes_pk4c(nodes, node_count, triangle_count, nd4c, &need4c, &H.refit.map4c) && need4c <= RTX_MAX_STACK - 2;
    if (!wide) H.refit.map4.clear();
    if (!wide_closest) H.refit.map4c.clear();
    // the distinct box-plane coordinates per axis, ascending: a ray with a zero direction component can only produce a NaN in a slab test
    // (0 * inf) if its origin lies exactly on one of them (pk_nan_possible, rtx_packet.h)
    std::vector<float> planes[3];
    for (int a = 0; a < 3; a++) {
        planes[a].reserve((size_t)node_count * 2);
        for (int i = 0; i < node_count; i++) { planes[a].push_back(nodes[i].aabb_min[a]); planes[a].push_back(nodes[i].aabb_max[a]); }
        planes[a].erase(std::remove_if(planes[a].begin(), planes[a].end(), [](float v) { return v != v; }), planes[a].end());
        std::sort(planes[a].begin(), planes[a].end());
        planes[a].erase(std::unique(planes[a].begin(), planes[a].end()), planes[a].end());      // +0 and -0 compare equal: one entry
        if (planes[a].empty()) planes[a].push_back(INFINITY);
    }
    DevBlas & B = S.B;
    memset(&B, 0, sizeof(B));
    int rc = RTX_OK;
    for (int a = 0; a < 3 && !rc; a++) { rc = stage_array(c, H.arrays, planes[a].data(), planes[a].size() * 4, planes[a].size() * 4, &B.planes[a]); B.plane_count[a] = (int32_t)planes[a].size(); }
    if (!rc && wide_closest) rc = stage_array(c, H.arrays, nd4c.data(), nd4c.size() * 16, nd4c.size() * 16, &B.pk4c_nodes);
    if (!rc && wide) rc = stage_array(c, H.arrays, nd4.data(), nd4.size() * 16, nd4.size() * 16, &B.pk4_nodes);
    if (!rc) rc = stage_array(c, H.arrays, nd.data(), nd.size() * 16, nd.size() * 16, &B.nodes);
    if (!rc) rc = stage_array(c, H.arrays, ndp.data(), ndp.size() * 16, ndp.size() * 16, &B.pk_nodes);
    if (!rc) rc = stage_array(c, H.arrays, th.data(), th.size() * 16, th.size() * 16, &B.tri_hot);
    if (!rc) rc = stage_array(c, H.arrays, tri_cold, (size_t)triangle_count * sizeof(rtx_triangle_cold), (size_t)(triangle_count > 0 ? triangle_count : 1) * sizeof(rtx_triangle_cold), &B.tri_cold);
    if (rc) return rc;
    B.node_count = node_count; B.tri_count = triangle_count; B.material_offset = material_offset; B.pk4_need = wide ? need4 : -1; B.pk4c_need = wide_closest ? need4c : -1;
    H.max_local_material = max_local;
    H.inner_depth = inner_depth;
    // the packet kernels pack stack entries and address nodes / triangles with 32-bit byte offsets (rtx_packet.h)
    H.packet_ok = leaf_max < 65536 && node_count < (1 << 26) && triangle_count < (1 << 25);
    return RTX_OK;
}

extern "C" int rtx_upload_blas(rtx_ctx * c, int32_t blas_id, const rtx_bvh_node * nodes, int32_t node_count,
                               const rtx_triangle_hot * tri_hot, const rtx_triangle_cold * tri_cold,
                               int32_t triangle_count, int32_t material_offset) {
    BlasStaged S;      // uploading an id drops its vertex binding and what rtx_alloc_blas made of it: the staged record has neither
    if (int rc = stage_blas(c, blas_id, nodes, node_count, tri_hot, tri_cold, triangle_count, material_offset, c ? c->knobs.pk4_order : 0, S)) return rc;
    return commit_blas(c, blas_id, S);
}

extern "C" int rtx_upload_materials(rtx_ctx * c, const rtx_material * materials, int32_t count) {
    if (!c || !materials || count <= 0) return RTX_ERR_INVALID_ARG;
    if (count > RTX_MAX_MATERIALS) return RTX_ERR_LIMIT;       // "Max Material limit reached!" Material.h:33-37
    hipSetDevice(c->cfg.device);
    return replace_table(c, c->d_materials, materials, (size_t)count * sizeof(rtx_material), [&] {
        c->material_count = count;
        c->h_materials.assign(materials, materials + count); c->refs_dirty = true;
    });
}

// texture_id now holds the texel array d with the descriptor desc: rtx_upload_texture and rtx_alloc_texture end here
static int commit_texture(rtx_ctx * c, int32_t texture_id, const rtx_texture_desc & desc, DevBuf & d, const rtx_ctx::TexUpdate & update) {
    std::vector<DevTexture> table = c->h_tex;
    if ((size_t)texture_id >= table.size()) { DevTexture none; memset(&none, 0, sizeof(none)); table.resize(texture_id + 1, none); }
    table[texture_id].desc = desc;
    table[texture_id].texels = (const float4 *)d.p;
    // replace_table waits for the stream first: the table is rewritten, and on a re-upload of an id the old texel array is released, after
    // the frames that may still read them
    return replace_table(c, c->d_textures, table.data(), table.size() * sizeof(DevTexture), [&] {
        c->h_tex.swap(table);
        if (c->tex_texels.size() < c->h_tex.size()) { c->tex_texels.resize(c->h_tex.size()); c->tex_update.resize(c->h_tex.size()); }
        c->tex_texels[texture_id] = std::move(d);
        c->tex_update[texture_id] = update;
        c->refs_dirty = true;
    });
}

extern "C" int rtx_upload_texture(rtx_ctx * c, int32_t texture_id, const rtx_texture_desc * desc, const float * texels_rgb, int64_t texel_count) {
    if (!c || texture_id < 0 || texture_id >= 4096 || !desc || !texels_rgb) return RTX_ERR_INVALID_ARG;
    if (desc->width <= 0 || desc->height <= 0 || desc->mip_levels < 1 || desc->mip_levels > RTX_MAX_MIP_LEVELS) return RTX_ERR_INVALID_ARG;
    for (int l = 0; l < desc->mip_levels; l++) {
        const int64_t lw = desc->width >> l, lh = desc->height >> l;
        if (lw < 1 || lh < 1 || desc->mip_offsets[l] < 0 || desc->mip_offsets[l] + lw * lh > texel_count) return RTX_ERR_INVALID_ARG;
    }
    hipSetDevice(c->cfg.device);
    DevBuf d;
    {   // float3 texels of the ABI -> one float4 per texel on the device
        std::vector<float4> padded((size_t)texel_count);
        for (int64_t i = 0; i < texel_count; i++) padded[(size_t)i] = make_float4(texels_rgb[3 * i], texels_rgb[3 * i + 1], texels_rgb[3 * i + 2], 0.0f);
        if (int rc = upload(c, d, padded.data(), (size_t)texel_count * 16)) return rc;
    }
    return commit_texture(c, texture_id, *desc, d, rtx_ctx::TexUpdate());
}

extern "C" int rtx_upload_sky(rtx_ctx * c, const float * texels_rgb, int32_t size) {
    if (!c || !texels_rgb || size <= 0 || size > 16384) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    // Sky::sample clamps the texel index to size*size INCLUSIVE (Sky.cpp:45): one zero texel of padding
    std::vector<float> padded((size_t)size * size * 3 + 3, 0.0f);
    memcpy(padded.data(), texels_rgb, (size_t)size * size * 12);
    return replace_table(c, c->d_sky, padded.data(), padded.size() * 4, [&] { c->sky_size = size; c->sky_uploaded = true; });
}

extern "C" int rtx_set_frame(rtx_ctx * c, const rtx_frame * f) {
    if (!c || !f) return RTX_ERR_INVALID_ARG;
    if (f->tlas_node_count < 0 || f->instance_count < 0 || f->sphere_count < 0 || f->plane_count < 0 || f->tlas_index_count < 0 ||
        f->point_light_count < 0 || f->spot_light_count < 0 || f->directional_light_count < 0) return RTX_ERR_INVALID_ARG;
    if ((f->tlas_node_count && !f->tlas_nodes) || (f->instance_count && !f->instances) || (f->tlas_index_count && !f->tlas_indices) ||
        (f->sphere_count && !f->spheres) || (f->plane_count && !f->planes) || (f->point_light_count && !f->point_lights) ||
        (f->spot_light_count && !f->spot_lights) || (f->directional_light_count && !f->directional_lights)) return RTX_ERR_INVALID_ARG;
    if (f->instance_count >= (1 << 28) || f->sphere_count >= (1 << 28) || f->plane_count >= (1 << 28)) return RTX_ERR_LIMIT;
    hipSetDevice(c->cfg.device);
    // validate the TLAS against the instance table and the instances against the uploaded BLAS set
    int tlas_depth = -1;
    if (f->tlas_node_count > 0 && !validate_tree(f->tlas_nodes, f->tlas_node_count, f->tlas_index_count, &tlas_depth)) return RTX_ERR_INVALID_ARG;
    for (int i = 0; i < f->tlas_index_count; i++) if (f->tlas_indices[i] < 0 || f->tlas_indices[i] >= f->instance_count) return RTX_ERR_INVALID_ARG;
    for (int i = 0; i < f->instance_count; i++) {
        const int b = f->instances[i].blas_id;
        if (b < 0 || (size_t)b >= c->h_blas.size() || !c->h_blas[b].nodes) return RTX_ERR_STATE;
    }
    // A NaN or infinite cell makes every local ray of that instance non-finite, which the packet walks do not survive (rtx_trace.h,
    // ray_is_finite): refused here, before anything changes.  Finite cells can still overflow a far origin (an open limit).
    bool rigid = true;
    for (int i = 0; i < f->instance_count; i++) {
        if (!rtxu::matrix_finite(f->instances[i].world) || !rtxu::matrix_finite(f->instances[i].world_inv)) {
            c->err = "rtx_set_frame: instance " + std::to_string(i) + " has a NaN or infinite world / world_inv cell"; return RTX_ERR_INVALID_ARG;
        }
        rigid = rigid && rtxu::instance_rigid(f->instances[i].world, f->instances[i].world_inv);
    }
    // Pack the frame into one block: [TLAS nodes, lane layout][TLAS nodes, packet layout][indices][instances][spheres][planes][lights],
    // every part 256-byte aligned.  The block is staged in pinned memory and copied by ONE hipMemcpyAsync on the context's stream: it is
    // ordered after the frames already queued there (which still read the previous contents) and before the next render call.
    std::vector<float4> nd, ndp; convert_nodes(f->tlas_nodes, f->tlas_node_count, nd); convert_nodes_pk(f->tlas_nodes, f->tlas_node_count, ndp);
    const void * src[9] = { nd.data(), ndp.data(), f->tlas_indices, f->instances, f->spheres, f->planes, f->point_lights, f->spot_lights, f->directional_lights };
    const size_t len[9] = { nd.size() * 16, ndp.size() * 16, (size_t)f->tlas_index_count * 4, (size_t)f->instance_count * sizeof(rtx_instance),
                            (size_t)f->sphere_count * sizeof(rtx_sphere), (size_t)f->plane_count * sizeof(rtx_plane), (size_t)f->point_light_count * sizeof(rtx_point_light),
                            (size_t)f->spot_light_count * sizeof(rtx_spot_light), (size_t)f->directional_light_count * sizeof(rtx_directional_light) };
    size_t off[9], total = 0;
    for (int k = 0; k < 9; k++) { off[k] = total; total += (len[k] + 255) & ~(size_t)255; if (len[k] == 0) total += 256; }
    int rc = RTX_OK;
    if (total > c->d_frame.cap) {                           // growth (first frame, or more instances than ever before): the one case that waits
        HIP_OK(c, hipStreamSynchronize(c->stream));
        rc = ensure(c, c->d_frame, total + total / 2);
        if (rc) return rc;
    }
    rc = stage_copy(c, c->frame_ring, c->d_frame.p, total, total + total / 2, [&](void * host) { for (int k = 0; k < 9; k++) if (len[k]) memcpy((char *)host + off[k], src[k], len[k]); });
    if (rc) return rc;
    char * const fb = (char *)c->d_frame.p;

    DevScene & s = c->scene;
    s.width = c->cfg.width; s.height = c->cfg.height; s.bounces = c->cfg.bounces; s.stack_size = c->cfg.stack_size;
    s.traversal_strategy = c->cfg.traversal_strategy; s.texture_mode = c->cfg.texture_mode; s.mip_filter = c->cfg.mip_filter;
    s.heatmap = c->cfg.heatmap ? 1 : 0;
    s.diff_enabled = c->cfg.texture_mode == RTX_TEXTURE_MIPMAP;            // RAY_DIFFERENTIALS_ENABLED, Config.h:46
    s.max_anisotropy = c->cfg.max_anisotropy;
    s.tile_count_x = (c->cfg.width + RTX_TILE_SIZE - 1) / RTX_TILE_SIZE;   // Window.cpp:11
    memcpy(s.cam_pos, f->camera.position, 12); memcpy(s.cam_tl, f->camera.rotated_top_left_corner, 12);
    memcpy(s.cam_x, f->camera.rotated_x_axis, 12); memcpy(s.cam_y, f->camera.rotated_y_axis, 12);
    memcpy(s.ambient, f->ambient, 12);
    bind_tables(c);                 // BLAS, materials, textures, sky: the same binding every later change of a table ends with (replace_table)
    s.ewa_table = (const float *)c->d_ewa.p;
    s.tlas_nodes = (const float4 *)(fb + off[0]); s.tlas_node_count = f->tlas_node_count; s.pk_tlas_nodes = (const float4 *)(fb + off[1]);
    s.tlas_indices = (const int32_t *)(fb + off[2]); s.tlas_index_count = f->tlas_index_count;
    s.instances = (const rtx_instance *)(fb + off[3]); s.instance_count = f->instance_count;
    s.spheres = (const rtx_sphere *)(fb + off[4]); s.sphere_count = f->sphere_count;
    s.planes = (const rtx_plane *)(fb + off[5]); s.plane_count = f->plane_count;
    s.point_lights = (const rtx_point_light *)(fb + off[6]); s.point_light_count = f->point_light_count;
    s.spot_lights = (const rtx_spot_light *)(fb + off[7]); s.spot_light_count = f->spot_light_count;
    s.dir_lights = (const rtx_directional_light *)(fb + off[8]); s.dir_light_count = f->directional_light_count;
    s.light_count = f->point_light_count + f->spot_light_count + f->directional_light_count;
    c->frame_primitive_materials.clear();
    for (int i = 0; i < f->sphere_count; i++) c->frame_primitive_materials.push_back(f->spheres[i].material_id);
    for (int i = 0; i < f->plane_count; i++) c->frame_primitive_materials.push_back(f->planes[i].material_id);
    c->tlas_inner_depth = tlas_depth;
    c->frame_set = true; c->refs_dirty = true; c->frame_rigid = rigid;
    c->frame_lone = plan_lone_facts(f->instance_count, f->tlas_nodes, f->tlas_node_count, f->tlas_indices, f->tlas_index_count, f->instances);
    s.lone = c->knobs.lone_entry && c->frame_lone.lone; s.copy_class = s.lone && c->frame_lone.copy_class;
    return RTX_OK;
}

// Every index a kernel dereferences without a bounds check of its own — material ids of primitives and triangles, texture ids of
// materials — is verified here, once after any upload / rtx_set_frame: a wrong id must become a status code, not a GPU memory fault.
static int validate_references(rtx_ctx * c) {
    if (!c->refs_dirty) return RTX_OK;
    const int nm = c->material_count;
    for (int id : c->frame_primitive_materials) if (id < 0 || id >= nm) { c->err = "sphere / plane material id outside the uploaded material table"; return RTX_ERR_STATE; }
    for (size_t b = 0; b < c->h_blas.size(); b++) {
        if (!c->h_blas[b].nodes) continue;
        const int hi = c->blas[b].max_local_material;
        if (c->h_blas[b].material_offset < 0 || (hi >= 0 && (long long)c->h_blas[b].material_offset + hi >= nm)) { c->err = "BLAS material_offset + triangle material id outside the uploaded material table"; return RTX_ERR_STATE; }
    }
    // BVH_TRAVERSAL_STACK_SIZE (Config.h:25).  The reference's per-BVH stack holds one pending sibling per ancestor entered through its near
    // child plus the two children pushed while a node is expanded (BottomLevelBVH.cpp:381-387, TopLevelBVH.cpp:76-82) and is not checked:
    // a tree with an inner node at depth d overflows a stack of fewer than d + 2 entries for some ray.  Such a tree is refused here,
    // for every ray alike.  The per-lane kernels' stacks (64 entries per BVH) can then never overflow; the packet kernels share one 64-entry
    // stack between TLAS and BLAS, and render_tiles_impl hands scenes that could exceed it to the per-lane kernels.
    for (size_t b = 0; b < c->h_blas.size(); b++)
        if (c->h_blas[b].nodes && c->blas[b].inner_depth + 2 > c->cfg.stack_size) {
            c->err = "BVH deeper than rtx_config.stack_size allows (BVH_TRAVERSAL_STACK_SIZE, Config.h:25): an inner node at depth " + std::to_string(c->blas[b].inner_depth) + " needs " + std::to_string(c->blas[b].inner_depth + 2) + " stack entries";
            return RTX_ERR_LIMIT;
        }
    if (c->tlas_inner_depth + 2 > c->cfg.stack_size) { c->err = "TLAS deeper than rtx_config.stack_size allows (BVH_TRAVERSAL_STACK_SIZE, Config.h:25)"; return RTX_ERR_LIMIT; }
    for (size_t i = 0; i < c->h_materials.size(); i++) {
        const int t = c->h_materials[i].texture_id;
        if (t >= 0 && ((size_t)t >= c->h_tex.size() || !c->h_tex[t].texels)) { c->err = "material refers to a texture id that was never uploaded"; return RTX_ERR_STATE; }
    }
    c->refs_dirty = false;
    return RTX_OK;
}

// ---- queue memory ------------------------------------------------------------------------------------
static int plan_batch(rtx_ctx * c, int tiles, int & out_tiles) {
    // worst case: every hit spawns two children -> level d holds P * 2^d rays
    const int levels = c->cfg.bounces + 1;
    const long long per_tile = 1024ll * ((1ll << levels) - 1);
    const long long budget = c->knobs.slot_budget;          // RTX_SLOT_BUDGET: tests force multi-batch frames with a small budget
    long long t = budget / per_tile;
    if (t < 1) t = 1;
    out_tiles = (int)(t < tiles ? t : tiles);
    return RTX_OK;
}

static int alloc_queues(rtx_ctx * c, int batch_tiles) {
    const int levels = c->cfg.bounces + 1;
    const long long P = 1024ll * batch_tiles;
    long long total = 0;
    // fused shading hands out the slots of levels >= 1 in wave-private chunks (rtx_packet.h RTX_PK_CHUNK): every wave of the launch above may leave one partly used
    const long long chunk_slack = c->knobs.fuse_shade ? (long long)c->pk_blocks_closest * (RTX_PK_BLOCK / RTX_WAVE) * RTX_PK_CHUNK : 0;
    for (int d = 0; d <= RTX_MAX_LEVELS; d++) {
        long long cap = d < levels ? (P << d) + (d > 0 ? chunk_slack : 0) : 0;
        c->q.level_base[d] = (int32_t)total; c->q.level_cap[d] = (int32_t)cap;
        total += cap;
    }
    if (total >= (1ll << 31)) { c->err = "batch too large"; return RTX_ERR_LIMIT; }
    const int nL = c->scene.light_count;
    long long stotal = 0;
    for (int d = 0; d <= RTX_MAX_LEVELS; d++) { c->q.shadow_base[d] = (int32_t)stotal; stotal += (long long)c->q.level_cap[d] * nL; }
    if (stotal >= (1ll << 31)) { c->err = "shadow queue too large"; return RTX_ERR_LIMIT; }
    const size_t slots = (size_t)total, sslots = (size_t)(stotal > 0 ? stotal : 1);
    int rc = 0, k = 0;
    // rays of level 0 are never stored, but the arrays are indexed by global slot for simplicity of addressing
    void ** f4[] = { (void **)&c->q.r0, (void **)&c->q.r1, (void **)&c->q.r2, (void **)&c->q.r3, (void **)&c->q.r4, (void **)&c->q.h0,
                     (void **)&c->q.n0, (void **)&c->q.n1, (void **)&c->q.n2, (void **)&c->q.c0, (void **)&c->q.c1,
                     (void **)&c->q.sp, (void **)&c->q.sn };
    for (void ** p : f4) { if (!rc) rc = ensure(c, c->qb[k], slots * 16); *p = c->qb[k].p; k++; }
    if (!rc) rc = ensure(c, c->qb[k], slots * 4); c->q.h1 = (int32_t *)c->qb[k].p; k++;
    c->q.views = nullptr; c->q.s0 = c->q.s1 = nullptr; c->q.shadow_explicit = 0; c->q.cull = 0;
    if (!rc) rc = ensure(c, c->qb[k], sslots * 4); c->q.socc = (uint32_t *)c->qb[k].p; k++;
    c->q.spill = (int32_t *)c->d_spill.p;
    c->q.counters = (DevCounters *)c->d_counters.p;
    c->q.pk_heads = (uint32_t *)c->d_pk_heads.p;
    c->q.pk_fifo = (int32_t *)c->d_pk_fifo.p;
    c->q.fb_rgb = (float *)(c->ext_rgb ? c->ext_rgb : c->d_fb_rgb.p);
    c->q.fb_packed = (uint32_t *)(c->ext_packed ? c->ext_packed : c->d_fb_packed.p);
    return rc;
}

__global__ void k_begin_batch(DevCounters * ctr, uint32_t * pk_heads, uint32_t primary_slots, uint32_t closest_threads, uint32_t any_threads,
                              uint32_t pk_waves_closest, uint32_t pk_waves_any, int first_batch) {
    // the first batch of a render call zeroes the whole counter block (stats of this call, WorkerThread.cpp:120) — done here rather than
    // with hipMemsetAsync, whose blit serialises the streams of different contexts against each other; every batch then resets the
    // queue state: the dynamic-fetch heads start behind the statically assigned first round (one ray per resident thread)
    const int i = threadIdx.x;
    if (first_batch) {
        uint32_t * w = reinterpret_cast<uint32_t *>(ctr);
        for (int k = i; k < (int)(sizeof(DevCounters) / 4); k += blockDim.x) w[k] = 0u;
        __syncthreads();
    }
    if (i <= RTX_MAX_LEVELS) { ctr->ray_count[i] = (i == 0) ? primary_slots : 0u; ctr->item_max[i] = 0u; ctr->fetch_closest[i] = closest_threads; ctr->fetch_any[i] = any_threads; }
    // packet-queue heads (rtx_packet.h): head c of a launch hands out packets k * 8 + c; the static first round (wave w takes packet w)
    // has already covered k < waves / 8 of every head
    for (int k = i; k < 2 * (RTX_MAX_LEVELS + 1) * RTX_PK_CLASSES; k += blockDim.x)
        pk_heads[k * 32] = (k < (RTX_MAX_LEVELS + 1) * RTX_PK_CLASSES ? pk_waves_closest : pk_waves_any) / RTX_PK_CLASSES;
}

static hipEvent_t next_event(rtx_ctx * c) {
    if (c->event_next == c->event_pool.size()) { hipEvent_t e; hipEventCreate(&e); c->event_pool.push_back(e); }
    return c->event_pool[c->event_next++];
}

// Packets by descending cost: a counting sort over 256 linear cost classes in ONE workgroup (32 400 packets at 1080p: ~10 us, on a side stream).
// The order inside a class is whatever the atomics make it — it is a schedule, not a result.
__global__ __launch_bounds__(1024) void k_packet_order(const uint32_t * __restrict__ cost, uint32_t * __restrict__ order, const uint32_t n) {
    __shared__ uint32_t hist[256], base[256];
    for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    auto cls = [](uint32_t c) { const uint32_t k = c >> 7; return 255u - (k < 255u ? k : 255u); };      // class 0 = the most expensive
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) atomicAdd(&hist[cls(cost[i])], 1u);
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t acc = 0; for (int k = 0; k < 256; k++) { base[k] = acc; acc += hist[k]; } }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) order[atomicAdd(&base[cls(cost[i])], 1u)] = i;
}

template <typename F>
static void launch_timed(rtx_ctx * c, const char * name, hipStream_t stream, F && launch) {
    if (c->timing) {
        KernelTime kt; kt.name = name; kt.a = next_event(c); kt.b = next_event(c);
        hipEventRecord(kt.a, stream);                 // events on the stream the kernel is launched on
        launch();
        hipEventRecord(kt.b, stream);
        c->times.push_back(kt);
    } else launch();
}

// k_begin_batch with the context's grid sizes: plain = the batch is traced by the plain kernels (one grid for both ray kinds)
static void begin_batch(rtx_ctx * c, DevCounters * counters, uint32_t * pk_heads, uint32_t primary_slots, bool plain, bool first_batch) {
    hipLaunchKernelGGL(k_begin_batch, dim3(1), dim3(64), 0, c->stream, counters, pk_heads, primary_slots,
                       (uint32_t)((plain ? c->trace_blocks_count : c->trace_blocks_closest) * RTX_TRACE_BLOCK),
                       (uint32_t)((plain ? c->trace_blocks_count : c->trace_blocks_any) * RTX_TRACE_BLOCK),
                       (uint32_t)(c->pk_blocks_closest * (RTX_PK_BLOCK / RTX_WAVE)), (uint32_t)(c->pk_blocks_any * (RTX_PK_BLOCK / RTX_WAVE)), first_batch ? 1 : 0);
}

// the two launches of a ray query's round (the debug hooks run the same rounds): the level-1 closest-hit walk and the level-0 shadow-ray walk, per lane or by packets
static void launch_closest_level1(rtx_ctx * c, const DevScene & sc, const DevQueues & q, bool lane) {
    if (lane) hipLaunchKernelGGL((k_trace_fast<false>), dim3(c->trace_blocks_closest), dim3(RTX_TRACE_BLOCK), 0, c->stream, sc, q, 1, 1);
    else      hipLaunchKernelGGL((k_packet<false, false>), dim3(c->pk_blocks_closest), dim3(RTX_PK_BLOCK), 0, c->stream, sc, q, 1, 1);
}
static void launch_any_level0(rtx_ctx * c, const DevScene & sc, const DevQueues & q, bool lane) {
    if (lane) hipLaunchKernelGGL((k_trace_fast<true>), dim3(c->trace_blocks_any), dim3(RTX_TRACE_BLOCK), 0, c->stream, sc, q, 0, 0);
    else      hipLaunchKernelGGL((k_packet<true, false>), dim3(c->pk_blocks_any), dim3(RTX_PK_BLOCK), 0, c->stream, sc, q, 0, 0);
}

// tiles of one frame (Window.cpp:11), and whether every uploaded mesh has 4-wide shadow-ray records (the split walk needs them)
static int32_t frame_tiles(const rtx_ctx * c) { return ((c->cfg.width + RTX_TILE_SIZE - 1) / RTX_TILE_SIZE) * ((c->cfg.height + RTX_TILE_SIZE - 1) / RTX_TILE_SIZE); }
static bool all_meshes_wide(const rtx_ctx * c) {
    for (const DevBlas & b : c->h_blas) if (b.nodes && !b.pk4_nodes) return false;
    return true;
}

// ---- what the device-side builders below share on the host ------------------------------------------------------------------------------
// n parts of one block, every part 256-byte aligned: off[k] = where part k of len[k] bytes starts; returns the block's size
static size_t aligned_parts(const size_t * len, size_t * off, int n) {
    size_t total = 0;
    for (int k = 0; k < n; k++) { off[k] = total; total += (len[k] + 255) & ~(size_t)255; }
    return total;
}

// rocPRIM's temporary storage for a radix sort of `count` keys of type Key over `bits` bits: a host-side query, nothing is launched
template <typename Key> static int sort_storage_bytes(rtx_ctx * c, size_t count, unsigned int bits, size_t & bytes) {
    bytes = 0;
    if (rocprim::radix_sort_keys(nullptr, bytes, (const Key *)nullptr, (Key *)nullptr, (unsigned int)count, 0u, bits, c->stream) == hipSuccess) return RTX_OK;
    hipGetLastError(); c->err = "rocprim::radix_sort_keys size query failed"; return RTX_ERR_HIP;
}

// a sort that failed: the sticky error is cleared, the context says why
static int sort_failed(rtx_ctx * c, hipError_t se) {
    hipGetLastError(); c->err = std::string("rocprim::radix_sort_keys: ") + hipGetErrorString(se); return RTX_ERR_HIP;
}

// a lane-layout array of n nodes in device memory back into the reference's records
static int read_lane_nodes(rtx_ctx * c, const float4 * dev, int n, rtx_bvh_node * out) {
    std::vector<float4> nd((size_t)2 * n);
    HIP_OK(c, hipMemcpy(nd.data(), dev, nd.size() * 16, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) rtxl::node_from_lane(nd.data(), i, out[i]);
    return RTX_OK;
}

// ---- device-side scene update (include/rtx.h: rtx_update_instances / rtx_read_frame_state; kernels in rtx_update.h) -------------------
// The instance records, the TLAS in both node layouts and its indices are rebuilt from poses in device memory into a block of their own
// (d_upd), and the DevScene pointers are switched to it; spheres, planes, lights and the camera stay where rtx_set_frame put them.  Everything
// is queued on the context's stream: work queued before keeps the state it was queued with (DevScene travels by value; a render call ends
// with the shadow-ray stream joined back into the context's stream, so the kernels here run after every reader of the block's previous
// contents), the next render call reads the new state.  The shape of the tree is a function of the instance count, so the depth the
// stack rules need (validate_references, render_tiles_impl) is known here without a read-back.  Nothing waits for the device except
// growth of the block (the first call, or more instances than ever before) — the case rtx_set_frame waits in too.
extern "C" int rtx_update_instances(rtx_ctx * c, const void * positions_dev, const void * rotations_dev, int32_t instance_count) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!positions_dev || !rotations_dev || ((uintptr_t)positions_dev & 3) || ((uintptr_t)rotations_dev & 3) || instance_count < 1) {
        c->err = "rtx_update_instances: null or misaligned pose pointer, or no instances"; return RTX_ERR_INVALID_ARG; }
    if (instance_count > RTX_UPDATE_MAX_INSTANCES) { c->err = "rtx_update_instances supports up to 65 536 instances"; return RTX_ERR_LIMIT; }
    if (!c->frame_set) { c->err = "rtx_update_instances before rtx_set_frame"; return RTX_ERR_STATE; }
    if (instance_count != c->scene.instance_count) { c->err = "rtx_update_instances: instance_count differs from the frame's"; return RTX_ERR_INVALID_ARG; }
    // the tree's depth is a function of the count: a tree the configured stack cannot hold (validate_references' rule) is refused here, before
    // anything is queued or switched, and the frame state stays what it was
    if (rtxu::tree_inner_depth(instance_count) + 2 > c->cfg.stack_size) {
        c->err = "rtx_update_instances: the balanced TLAS of " + std::to_string(instance_count) + " instances needs " + std::to_string(rtxu::tree_inner_depth(instance_count) + 2) +
                 " stack entries, rtx_config.stack_size allows fewer (BVH_TRAVERSAL_STACK_SIZE, Config.h:25)";
        return RTX_ERR_LIMIT;
    }
    hipSetDevice(c->cfg.device);
    const int n = instance_count, levels = rtxu::tree_levels(n), slots = rtxu::tree_node_count(n);
    const bool small = n <= c->knobs.update_small_max;
    // [nodes, lane layout][nodes, packet layout][indices][instances][AABBs][sorted keys][bounds], every part 256-byte aligned
    const size_t len[7] = { (size_t)slots * 32, (size_t)slots * 32, (size_t)n * 4, (size_t)n * sizeof(rtx_instance), (size_t)n * 24, (size_t)n * 8, 24 };
    size_t off[7];
    const size_t total = aligned_parts(len, off, 7);
    if (n > c->upd_cap || total > c->d_upd.cap) {           // growth: never while the scene points into the block (the count is the frame's, the block holds it)
        HIP_OK(c, hipStreamSynchronize(c->stream));
        if (int rc = ensure(c, c->d_upd, total)) return rc;
        c->upd_cap = n;
    }
    size_t sort_bytes = 0;
    if (!small) {                                           // rocPRIM's temporary storage, sized for this n by a host-side query; grown only
        if (int rc = sort_storage_bytes<uint64_t>(c, (size_t)n, RTXU_KEY_BITS, sort_bytes)) return rc;
        const size_t keys_in = ((size_t)n * 8 + 255) & ~(size_t)255;
        if (keys_in + sort_bytes > c->d_upd_sort.cap) {
            HIP_OK(c, hipStreamSynchronize(c->stream));
            if (int rc = ensure(c, c->d_upd_sort, keys_in + sort_bytes)) return rc;
        }
    }
    char * const ub = (char *)c->d_upd.p;
    DevUpdate u;
    u.positions = (const float *)positions_dev; u.rotations = (const float *)rotations_dev;
    u.src_instances = c->scene.instances; u.blas = c->scene.blas;
    u.nodes = (float4 *)(ub + off[0]); u.pk_nodes = (float4 *)(ub + off[1]); u.indices = (int32_t *)(ub + off[2]);
    u.instances = (rtx_instance *)(ub + off[3]); u.aabbs = (float *)(ub + off[4]); u.keys = (uint64_t *)(ub + off[5]); u.bounds = (uint32_t *)(ub + off[6]);
    u.n = n; u.levels = levels;
    if (small) {
        launch_timed(c, "k_update_small", c->stream, [&] { hipLaunchKernelGGL(k_update_small, dim3(1), dim3(RTX_UPDATE_BLOCK), 0, c->stream, u); });
    } else {
        uint64_t * const keys_in = (uint64_t *)c->d_upd_sort.p;
        void * const sort_tmp = (char *)c->d_upd_sort.p + (((size_t)n * 8 + 255) & ~(size_t)255);
        const int blocks = (n + 255) / 256;
        HIP_OK(c, hipMemsetAsync(u.bounds, 0xff, 24, c->stream));
        launch_timed(c, "k_update_instances", c->stream, [&] { hipLaunchKernelGGL(k_update_instances, dim3(blocks), dim3(256), 0, c->stream, u); });
        launch_timed(c, "k_update_keys", c->stream, [&] { hipLaunchKernelGGL(k_update_keys, dim3(blocks), dim3(256), 0, c->stream, u, keys_in); });
        hipError_t se = hipSuccess;
        launch_timed(c, "update_radix_sort", c->stream, [&] { se = rocprim::radix_sort_keys(sort_tmp, sort_bytes, (const uint64_t *)keys_in, u.keys, (unsigned int)n, 0u, (unsigned int)RTXU_KEY_BITS, c->stream); });
        if (se != hipSuccess) return sort_failed(c, se);
        for (int d = levels; d > RTX_UPDATE_TOP_LEVELS; d--)
            launch_timed(c, "k_update_level", c->stream, [&] { hipLaunchKernelGGL(k_update_level, dim3(((1 << d) + 255) / 256), dim3(256), 0, c->stream, u, d); });
        launch_timed(c, "k_update_top", c->stream, [&] { hipLaunchKernelGGL(k_update_top, dim3(1), dim3(RTX_UPDATE_BLOCK), 0, c->stream, u); });
    }
    HIP_OK(c, hipGetLastError());
    DevScene & s = c->scene;
    s.tlas_nodes = u.nodes; s.pk_tlas_nodes = u.pk_nodes; s.tlas_node_count = slots;
    s.tlas_indices = u.indices; s.tlas_index_count = n; s.instances = u.instances;
    c->tlas_inner_depth = rtxu::tree_inner_depth(n);
    c->refs_dirty = true;
    c->frame_rigid = true;                                  // unit quaternions, by this call's contract: Mesh::update's poses
    c->frame_lone = LoneFacts{ false, false }; s.lone = 0; s.copy_class = 0;      // matrices the host has not seen: the general entry until the next rtx_set_frame
    return RTX_OK;
}

extern "C" int rtx_read_frame_state(rtx_ctx * c, rtx_instance * instances, rtx_bvh_node * tlas_nodes, int32_t * tlas_node_count, int32_t * tlas_indices) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!c->frame_set) { c->err = "rtx_read_frame_state before rtx_set_frame"; return RTX_ERR_STATE; }
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    const DevScene & s = c->scene;
    if (tlas_node_count) *tlas_node_count = s.tlas_node_count;
    if (instances && s.instance_count) HIP_OK(c, hipMemcpy(instances, s.instances, (size_t)s.instance_count * sizeof(rtx_instance), hipMemcpyDeviceToHost));
    if (tlas_indices && s.tlas_index_count) HIP_OK(c, hipMemcpy(tlas_indices, s.tlas_indices, (size_t)s.tlas_index_count * 4, hipMemcpyDeviceToHost));
    if (tlas_nodes && s.tlas_node_count) return read_lane_nodes(c, s.tlas_nodes, s.tlas_node_count, tlas_nodes);
    return RTX_OK;
}

// ---- device-side mesh refit (include/rtx.h: rtx_bind_blas_vertices / rtx_refit_blas / rtx_read_blas; kernels in rtx_refit.h) -----------
// Everything the host decides from a BLAS before a launch (inner_depth, packet_ok, pk4_need / pk4c_need, the packet-stack rule,
// the kernel choice per level) depends on its topology, which a refit keeps: so a refit is queued on the context's stream like
// rtx_update_instances and nothing is read back.  The arrays are written in place and the DevBlas table is not touched after the bind, so
// work queued before reads the old mesh, the next render call the new one, and a captured graph stays valid.
static int refit_launch_finish(rtx_ctx * c, rtx_ctx::BlasRefit & R, bool build = false) {
    const DevRefit & r = R.dev;
    const int n = r.node_count;
    const dim3 grid((2 * n + 4 + RTX_REFIT_BLOCK - 1) / RTX_REFIT_BLOCK);
    if (build) launch_timed(c, "k_build_finish", c->stream, [&] { hipLaunchKernelGGL(k_build_finish, grid, dim3(RTX_REFIT_BLOCK), 0, c->stream, r); });      // + the axis fields
    else launch_timed(c, "k_refit_finish", c->stream, [&] { hipLaunchKernelGGL(k_refit_finish, grid, dim3(RTX_REFIT_BLOCK), 0, c->stream, r); });
    hipError_t se = hipSuccess;
    launch_timed(c, "refit_plane_sort", c->stream, [&] {
        for (int a = 0; a < 3 && se == hipSuccess; a++) {
            size_t bytes = R.sort_bytes;
            se = rocprim::radix_sort_keys(R.sort_tmp, bytes, (const float *)r.plane_keys[a], R.planes[a], (unsigned int)(2 * n), 0u, 32u, c->stream);
        }
    });
    if (se != hipSuccess) return sort_failed(c, se);
    HIP_OK(c, hipGetLastError());
    return RTX_OK;
}

// The refit plan of a mesh: one device block, the kernel arguments that point into it, and the mesh's plane lists moved into it.  B and R are the
// caller's staged copies (R carries the slot maps of the upload); nothing of the context is written, so a failure changes nothing and the
// block dies with R.  The index table as given: rtx_bind_blas_vertices has validated it, rtx_alloc_blas hands in -1 everywhere (every
// triangle invalid until a build).
static int plan_refit(rtx_ctx * c, DevBlas & B, rtx_ctx::BlasRefit & R, const int32_t * slot_vertices, int32_t vertex_count) {
    const int n = B.node_count, T = B.tri_count;
    // the topology as uploaded: the lane layout's words (a refit never writes them)
    std::vector<float4> nd((size_t)2 * n);
    HIP_OK(c, hipMemcpy(nd.data(), B.nodes, nd.size() * 16, hipMemcpyDeviceToHost));
    std::vector<int32_t> parent;
    parent_table(nd.data(), n, parent);
    size_t sort_bytes = 0;
    if (int rc = sort_storage_bytes<float>(c, (size_t)2 * n, 32u, sort_bytes)) return rc;
    // [slot vertices][parents][arrival counters][pk4 slot map][pk4c slot map][3 x plane keys][3 x planes][sort storage], every part 256-byte aligned
    const size_t slots = (size_t)2 * n + 4, pl = (size_t)2 * n * 4;
    const size_t len[12] = { (size_t)(T > 0 ? T : 1) * 12, (size_t)n * 4, (size_t)n * 4, R.map4.empty() ? 0 : slots * 4, R.map4c.empty() ? 0 : slots * 4, pl, pl, pl, pl, pl, pl, sort_bytes };
    size_t off[12];
    if (int rc = ensure(c, R.block, aligned_parts(len, off, 12))) return rc;
    char * const bb = (char *)R.block.p;
    if (T) HIP_OK(c, hipMemcpy(bb + off[0], slot_vertices, (size_t)T * 12, hipMemcpyHostToDevice));
    HIP_OK(c, hipMemcpy(bb + off[1], parent.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_OK(c, hipMemset(bb + off[2], 0, (size_t)n * 4));
    if (!R.map4.empty()) HIP_OK(c, hipMemcpy(bb + off[3], R.map4.data(), slots * 4, hipMemcpyHostToDevice));
    if (!R.map4c.empty()) HIP_OK(c, hipMemcpy(bb + off[4], R.map4c.data(), slots * 4, hipMemcpyHostToDevice));
    DevRefit & r = R.dev;
    memset(&r, 0, sizeof(r));
    r.slot_vertices = (const int32_t *)(bb + off[0]); r.parent = (const int32_t *)(bb + off[1]); r.arrivals = (uint32_t *)(bb + off[2]);
    r.map4 = R.map4.empty() ? nullptr : (const int32_t *)(bb + off[3]); r.map4c = R.map4c.empty() ? nullptr : (const int32_t *)(bb + off[4]);
    for (int a = 0; a < 3; a++) r.plane_keys[a] = (float *)(bb + off[5 + a]);
    r.nodes = (float4 *)B.nodes; r.pk_nodes = (float4 *)B.pk_nodes; r.pk4_nodes = (float4 *)B.pk4_nodes; r.pk4c_nodes = (float4 *)B.pk4c_nodes;
    r.tri_hot = (float4 *)B.tri_hot; r.tri_cold = (float4 *)B.tri_cold;
    r.node_count = n; r.tri_count = T;
    R.sort_tmp = bb + off[11]; R.sort_bytes = sort_bytes;
    // the plane lists move into buffers of a fixed 2 * node_count floats, filled from the boxes the arrays hold now by the pass a refit ends with
    // (which also rewrites the packet and wide boxes with the values they already have): duplicates and the planes of unreachable slots only
    // send a ray to the reference-form walker (plane_member is a lower-bound search)
    for (int a = 0; a < 3; a++) { R.planes[a] = (float *)(bb + off[8 + a]); B.planes[a] = R.planes[a]; B.plane_count[a] = 2 * n; }
    const int rc = refit_launch_finish(c, R);
    const hipError_t waited = hipStreamSynchronize(c->stream);      // on failure too: what was queued writes the block the caller is about to drop
    if (rc) return rc;
    if (waited != hipSuccess) { c->err = std::string("hipStreamSynchronize: ") + hipGetErrorString(waited); return RTX_ERR_HIP; }
    R.bound = true; R.vertex_count = vertex_count;
    return RTX_OK;
}

extern "C" int rtx_bind_blas_vertices(rtx_ctx * c, int32_t blas_id, const int32_t * slot_vertices, int32_t vertex_count) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!slot_vertices || blas_id < 0 || blas_id >= (1 << 20) || vertex_count < 1) { c->err = "rtx_bind_blas_vertices: null index table, bad id or no vertices"; return RTX_ERR_INVALID_ARG; }
    if ((size_t)blas_id >= c->h_blas.size() || !c->h_blas[blas_id].nodes) { c->err = "rtx_bind_blas_vertices: no BLAS uploaded under that id"; return RTX_ERR_STATE; }
    const int64_t T3 = 3 * (int64_t)c->h_blas[blas_id].tri_count;
    for (int64_t k = 0; k < T3; k++) if (slot_vertices[k] < 0 || slot_vertices[k] >= vertex_count) {
        c->err = "rtx_bind_blas_vertices: vertex index outside [0, vertex_count)"; return RTX_ERR_INVALID_ARG; }
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));                    // frames in flight read the tables this call replaces
    rtx_ctx::BlasRefit & R = c->blas[blas_id].refit;
    if (R.bound) {                                                  // same arrays, same topology: only the index table changes
        if (T3) HIP_OK(c, hipMemcpy((void *)R.dev.slot_vertices, slot_vertices, (size_t)T3 * 4, hipMemcpyHostToDevice));
        R.vertex_count = vertex_count;
        return RTX_OK;
    }
    // the plan is made on copies and swapped in with the table: a failure leaves the id unbound, with the plane lists of its upload
    DevBlas B = c->h_blas[blas_id];
    rtx_ctx::BlasRefit N; N.map4 = R.map4; N.map4c = R.map4c;
    if (int rc = plan_refit(c, B, N, slot_vertices, vertex_count)) return rc;
    std::vector<DevBlas> table = c->h_blas;
    table[blas_id] = B;
    return upload_blas_table(c, table, [&] { c->blas[blas_id].refit = std::move(N); });
}

extern "C" int rtx_refit_blas(rtx_ctx * c, int32_t blas_id, const void * positions_dev, const void * normals_dev, int32_t vertex_count) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!positions_dev || ((uintptr_t)positions_dev & 3) || ((uintptr_t)normals_dev & 3)) { c->err = "rtx_refit_blas: null or misaligned vertex pointer"; return RTX_ERR_INVALID_ARG; }
    if (blas_id < 0 || (size_t)blas_id >= c->h_blas.size() || !c->h_blas[blas_id].nodes || !c->blas[blas_id].refit.bound) {
        c->err = "rtx_refit_blas: no BLAS uploaded under that id, or no vertices bound to it (rtx_bind_blas_vertices)"; return RTX_ERR_STATE; }
    rtx_ctx::BlasRefit & R = c->blas[blas_id].refit;
    if (vertex_count != R.vertex_count) { c->err = "rtx_refit_blas: vertex_count differs from the bound one"; return RTX_ERR_INVALID_ARG; }
    hipSetDevice(c->cfg.device);
    DevRefit & r = R.dev;
    r.positions = (const float *)positions_dev; r.normals = (const float *)normals_dev;
    const int n = r.node_count, T = r.tri_count;
    if (T) launch_timed(c, "k_refit_triangles", c->stream, [&] { hipLaunchKernelGGL(k_refit_triangles, dim3((T + RTX_REFIT_BLOCK - 1) / RTX_REFIT_BLOCK), dim3(RTX_REFIT_BLOCK), 0, c->stream, r); });
    launch_timed(c, "k_refit_climb", c->stream, [&] { hipLaunchKernelGGL(k_refit_climb, dim3((n + RTX_REFIT_BLOCK - 1) / RTX_REFIT_BLOCK), dim3(RTX_REFIT_BLOCK), 0, c->stream, r); });
    return refit_launch_finish(c, R);
}

// ---- device-side mesh build (include/rtx.h: rtx_alloc_blas / rtx_build_blas; kernels in rtx_build.h) -----------------------------------
// The balanced tree's topology is a function of the triangle count (rtx_build_math.h), so rtx_alloc_blas can do everything the host decides
// from a BLAS before a launch — inner_depth, packet_ok, pk4_need / pk4c_need, the 4-wide slot orders and maps, the refit plan — once,
// by handing the topology with all-zero boxes (nested, min <= max) to the code rtx_upload_blas and rtx_bind_blas_vertices run.  A build is then
// queued like a refit: it writes the arrays in place, touches no pointer and reads nothing back.
extern "C" int rtx_alloc_blas(rtx_ctx * c, int32_t blas_id, int32_t triangle_count, int32_t vertex_count, const int32_t * material_ids, int32_t material_offset) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (blas_id < 0 || blas_id >= (1 << 20) || triangle_count < 1 || vertex_count < 1) { c->err = "rtx_alloc_blas: bad id, no triangles or no vertices"; return RTX_ERR_INVALID_ARG; }
    int max_local = 0;
    if (material_ids) for (int i = 0; i < triangle_count; i++) {
        if (material_ids[i] < 0) { c->err = "rtx_alloc_blas: negative material id"; return RTX_ERR_INVALID_ARG; }
        if (material_ids[i] > max_local) max_local = material_ids[i];
    }
    if (triangle_count >= RTX_BUILD_MAX_TRIANGLES) { c->err = "rtx_alloc_blas supports fewer than 2^24 triangles (the 4-wide walks' limit)"; return RTX_ERR_LIMIT; }
    if (rtxb::tree_inner_depth(triangle_count) + 2 > c->cfg.stack_size) {
        c->err = "rtx_alloc_blas: the balanced BLAS of " + std::to_string(triangle_count) + " triangles needs " + std::to_string(rtxb::tree_inner_depth(triangle_count) + 2) +
                 " stack entries, rtx_config.stack_size allows fewer (BVH_TRAVERSAL_STACK_SIZE, Config.h:25)";
        return RTX_ERR_LIMIT;
    }
    hipSetDevice(c->cfg.device);
    const int T = triangle_count;
    std::vector<rtx_bvh_node> nodes;
    balanced_topology(T, nodes);
    BlasStaged S;                                                   // mesh, refit plan and build scratch are staged together and committed as one
    {   // zeroed triangle arrays: a zero triangle is hit by no ray, so the mesh is empty and legal to render until the first build
        std::vector<rtx_triangle_hot> hot((size_t)T); std::vector<rtx_triangle_cold> cold((size_t)T);
        memset(hot.data(), 0, hot.size() * sizeof(rtx_triangle_hot)); memset(cold.data(), 0, cold.size() * sizeof(rtx_triangle_cold));
        if (int rc = stage_blas(c, blas_id, nodes.data(), (int32_t)nodes.size(), hot.data(), cold.data(), T, material_offset, 0, S)) return rc;
    }
    S.H.max_local_material = max_local;                             // the ids a build will scatter into the cold records
    HIP_OK(c, hipStreamSynchronize(c->stream));
    {
        std::vector<int32_t> sv((size_t)3 * T, -1);
        if (int rc = plan_refit(c, S.B, S.H.refit, sv.data(), vertex_count)) return rc;
    }
    size_t sort_bytes = 0;
    if (int rc = sort_storage_bytes<uint64_t>(c, (size_t)T, RTXB_KEY_BITS, sort_bytes)) return rc;
    // [material ids][bounds][unsorted keys][sorted keys][sort storage], every part 256-byte aligned
    const size_t len[5] = { (size_t)T * 4, 24, (size_t)T * 8, (size_t)T * 8, sort_bytes };
    size_t off[5];
    rtx_ctx::BlasBuild & U = S.H.build;
    if (int rc = ensure(c, U.block, aligned_parts(len, off, 5))) return rc;
    char * const bb = (char *)U.block.p;
    if (material_ids) HIP_OK(c, hipMemcpy(bb + off[0], material_ids, (size_t)T * 4, hipMemcpyHostToDevice));
    else HIP_OK(c, hipMemset(bb + off[0], 0, (size_t)T * 4));
    memset(&U.dev, 0, sizeof(U.dev));
    U.dev.material_ids = (const int32_t *)(bb + off[0]); U.dev.bounds = (uint32_t *)(bb + off[1]);
    U.dev.keys_in = (uint64_t *)(bb + off[2]); U.dev.keys = (uint64_t *)(bb + off[3]);
    U.dev.slot_vertices = (int32_t *)S.H.refit.dev.slot_vertices;
    U.dev.tri_count = T; U.dev.vertex_count = vertex_count;
    U.sort_tmp = bb + off[4]; U.sort_bytes = sort_bytes; U.levels = rtxb::tree_levels(T);
    U.allocated = true;
    return commit_blas(c, blas_id, S);
}

extern "C" int rtx_build_blas(rtx_ctx * c, int32_t blas_id, const void * positions_dev, const void * indices_dev, const void * normals_dev,
                              const void * texcoords_dev, void * order_out_dev) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!positions_dev || !indices_dev || !normals_dev || (((uintptr_t)positions_dev | (uintptr_t)indices_dev | (uintptr_t)normals_dev | (uintptr_t)texcoords_dev | (uintptr_t)order_out_dev) & 3)) {
        c->err = "rtx_build_blas: null or misaligned pointer"; return RTX_ERR_INVALID_ARG; }
    if (blas_id < 0 || (size_t)blas_id >= c->blas.size() || !c->blas[blas_id].build.allocated) { c->err = "rtx_build_blas: the id was not created by rtx_alloc_blas"; return RTX_ERR_STATE; }
    hipSetDevice(c->cfg.device);
    rtx_ctx::BlasBuild & U = c->blas[blas_id].build;
    rtx_ctx::BlasRefit & R = c->blas[blas_id].refit;
    DevBuild & b = U.dev; DevRefit & r = R.dev;
    b.positions = (const float *)positions_dev; b.indices = (const int32_t *)indices_dev; b.normals = (const float *)normals_dev;
    b.texcoords = (const float *)texcoords_dev; b.order_out = (int32_t *)order_out_dev;
    r.positions = b.positions; r.normals = b.normals;
    const int T = b.tri_count;
    const dim3 tri_grid((T + RTX_BUILD_BLOCK - 1) / RTX_BUILD_BLOCK);
    HIP_OK(c, hipMemsetAsync(b.bounds, 0xff, 24, c->stream));
    launch_timed(c, "k_build_bounds", c->stream, [&] { hipLaunchKernelGGL(k_build_bounds, tri_grid, dim3(RTX_BUILD_BLOCK), 0, c->stream, b); });
    launch_timed(c, "k_build_keys", c->stream, [&] { hipLaunchKernelGGL(k_build_keys, tri_grid, dim3(RTX_BUILD_BLOCK), 0, c->stream, b); });
    hipError_t se = hipSuccess;
    launch_timed(c, "build_radix_sort", c->stream, [&] { size_t bytes = U.sort_bytes; se = rocprim::radix_sort_keys(U.sort_tmp, bytes, (const uint64_t *)b.keys_in, b.keys, (unsigned int)T, 0u, (unsigned int)RTXB_KEY_BITS, c->stream); });
    if (se != hipSuccess) return sort_failed(c, se);
    launch_timed(c, "k_build_scatter", c->stream, [&] { hipLaunchKernelGGL(k_build_scatter, tri_grid, dim3(RTX_BUILD_BLOCK), 0, c->stream, b, r); });
    for (int d = U.levels; d > RTX_BUILD_TOP_LEVELS; d--)
        launch_timed(c, "k_build_level", c->stream, [&] { hipLaunchKernelGGL(k_build_level, dim3(((1 << d) + RTX_BUILD_BLOCK - 1) / RTX_BUILD_BLOCK), dim3(RTX_BUILD_BLOCK), 0, c->stream, r, d); });
    launch_timed(c, "k_build_top", c->stream, [&] { hipLaunchKernelGGL(k_build_top, dim3(1), dim3(RTX_BUILD_TOP_BLOCK), 0, c->stream, r, U.levels); });
    return refit_launch_finish(c, R, true);
}

// ---- device-side vertex normals (include/rtx.h: rtx_alloc_blas_topology / rtx_set_blas_topology / rtx_blas_vertex_normals; kernels in
// rtx_normals.h) -------------------------------------------------------------------------------------------------------------------------
// The state lives in the id's host record, so whatever replaces the record (rtx_upload_blas, rtx_alloc_blas: commit_blas) drops it.  The
// alloc stages its block and swaps it in after waiting for the stream; the other two calls are queued like a refit and read nothing back.
extern "C" int rtx_alloc_blas_topology(rtx_ctx * c, int32_t blas_id, int32_t triangle_count, int32_t vertex_count) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (blas_id < 0 || blas_id >= (1 << 20) || triangle_count < 1 || vertex_count < 1) { c->err = "rtx_alloc_blas_topology: bad id, no triangles or no vertices"; return RTX_ERR_INVALID_ARG; }
    if (triangle_count > RTX_NORMALS_MAX_TRIANGLES) { c->err = "rtx_alloc_blas_topology supports at most 2^28 triangles (32-bit corner indices)"; return RTX_ERR_LIMIT; }
    if ((size_t)blas_id >= c->h_blas.size() || !c->h_blas[blas_id].nodes) { c->err = "rtx_alloc_blas_topology: no BLAS uploaded or allocated under that id"; return RTX_ERR_STATE; }
    hipSetDevice(c->cfg.device);
    const size_t T = (size_t)triangle_count, V = (size_t)vertex_count;
    rtx_ctx::BlasNormals N;
    N.key_bits = rtxn::key_bits(vertex_count);
    if (int rc = sort_storage_bytes<uint64_t>(c, 3 * T, N.key_bits, N.sort_bytes)) return rc;
    // [indices][unsorted keys][sorted keys][sort storage][offsets][face vectors], every part 256-byte aligned
    const size_t len[6] = { T * 12, 3 * T * 8, 3 * T * 8, N.sort_bytes, (V + 1) * 4, T * 16 };
    size_t off[6];
    if (int rc = ensure(c, N.block, aligned_parts(len, off, 6))) return rc;
    char * const bb = (char *)N.block.p;
    memset(&N.dev, 0, sizeof(N.dev));
    N.dev.indices = (int32_t *)(bb + off[0]); N.dev.keys_in = (uint64_t *)(bb + off[1]); N.dev.keys = (uint64_t *)(bb + off[2]);
    N.sort_tmp = bb + off[3]; N.dev.offset = (uint32_t *)(bb + off[4]); N.dev.face = (float4 *)(bb + off[5]);
    N.dev.tri_count = triangle_count; N.dev.vertex_count = vertex_count;
    N.allocated = true;
    HIP_OK(c, hipStreamSynchronize(c->stream));                    // queued normals still read the block this call replaces
    c->blas[blas_id].normals = std::move(N);
    c->blas[blas_id].side = rtx_ctx::BlasSide();                   // the pseudonormal tables were made over the replaced topology
    drop_side_entry(c, blas_id);
    return RTX_OK;
}

extern "C" int rtx_set_blas_topology(rtx_ctx * c, int32_t blas_id, const void * indices_dev) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!indices_dev || ((uintptr_t)indices_dev & 3)) { c->err = "rtx_set_blas_topology: null or misaligned index pointer"; return RTX_ERR_INVALID_ARG; }
    if (blas_id < 0 || (size_t)blas_id >= c->blas.size() || !c->blas[blas_id].normals.allocated) { c->err = "rtx_set_blas_topology: no topology allocated under that id (rtx_alloc_blas_topology)"; return RTX_ERR_STATE; }
    hipSetDevice(c->cfg.device);
    rtx_ctx::BlasNormals & N = c->blas[blas_id].normals;
    DevNormals & d = N.dev;
    d.indices_src = (const int32_t *)indices_dev;
    const uint32_t corners = 3u * (uint32_t)d.tri_count;
    launch_timed(c, "k_normals_keys", c->stream, [&] { hipLaunchKernelGGL(k_normals_keys, dim3((corners + RTX_NORMALS_BLOCK - 1) / RTX_NORMALS_BLOCK), dim3(RTX_NORMALS_BLOCK), 0, c->stream, d); });
    hipError_t se = hipSuccess;
    launch_timed(c, "normals_radix_sort", c->stream, [&] { size_t bytes = N.sort_bytes; se = rocprim::radix_sort_keys(N.sort_tmp, bytes, (const uint64_t *)d.keys_in, d.keys, (unsigned int)corners, 0u, N.key_bits, c->stream); });
    if (se != hipSuccess) return sort_failed(c, se);
    launch_timed(c, "k_normals_offsets", c->stream, [&] { hipLaunchKernelGGL(k_normals_offsets, dim3(((uint32_t)d.vertex_count + 1 + RTX_NORMALS_BLOCK - 1) / RTX_NORMALS_BLOCK), dim3(RTX_NORMALS_BLOCK), 0, c->stream, d); });
    HIP_OK(c, hipGetLastError());
    N.set = true;
    return RTX_OK;
}

extern "C" int rtx_blas_vertex_normals(rtx_ctx * c, int32_t blas_id, const void * positions_dev, void * normals_out_dev) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!positions_dev || !normals_out_dev || (((uintptr_t)positions_dev | (uintptr_t)normals_out_dev) & 3)) { c->err = "rtx_blas_vertex_normals: null or misaligned pointer"; return RTX_ERR_INVALID_ARG; }
    if (blas_id < 0 || (size_t)blas_id >= c->blas.size() || !c->blas[blas_id].normals.allocated) { c->err = "rtx_blas_vertex_normals: no topology allocated under that id (rtx_alloc_blas_topology)"; return RTX_ERR_STATE; }
    rtx_ctx::BlasNormals & N = c->blas[blas_id].normals;
    if (!N.set) { c->err = "rtx_blas_vertex_normals: no topology set since the alloc (rtx_set_blas_topology)"; return RTX_ERR_STATE; }
    hipSetDevice(c->cfg.device);
    DevNormals & d = N.dev;
    d.positions = (const float *)positions_dev; d.normals_out = (float *)normals_out_dev;
    launch_timed(c, "k_normals_faces", c->stream, [&] { hipLaunchKernelGGL(k_normals_faces, dim3(((uint32_t)d.tri_count + RTX_NORMALS_BLOCK - 1) / RTX_NORMALS_BLOCK), dim3(RTX_NORMALS_BLOCK), 0, c->stream, d); });
    launch_timed(c, "k_normals_sum", c->stream, [&] { hipLaunchKernelGGL(k_normals_sum, dim3(((uint32_t)d.vertex_count + RTX_NORMALS_BLOCK - 1) / RTX_NORMALS_BLOCK), dim3(RTX_NORMALS_BLOCK), 0, c->stream, d); });
    HIP_OK(c, hipGetLastError());
    return RTX_OK;
}

// ---- pseudonormal tables (include/rtx.h: rtx_blas_pseudonormals / rtx_read_blas_pseudonormals; kernels in rtx_side.h, arithmetic in
// rtx_side_math.h) ----------------------------------------------------------------------------------------------------------------------
// The state lives in the id's host record beside the topology it is made from.  The first call for an id stages its block, waits for the
// stream and swaps it in (a refused allocation changes nothing); later calls only queue the three kernels.  The kernels read the topology's
// block (indices, sorted keys, offsets) and the refit plan's slot table: whatever replaces either (commit_blas, rtx_alloc_blas_topology) drops
// this state with it.
extern "C" int rtx_blas_pseudonormals(rtx_ctx * c, int32_t blas_id, const void * positions_dev) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!positions_dev || ((uintptr_t)positions_dev & 3)) { c->err = "rtx_blas_pseudonormals: null or misaligned pointer"; return RTX_ERR_INVALID_ARG; }
    if (blas_id < 0 || (size_t)blas_id >= c->blas.size() || !c->blas[blas_id].normals.allocated) { c->err = "rtx_blas_pseudonormals: no topology allocated under that id (rtx_alloc_blas_topology)"; return RTX_ERR_STATE; }
    rtx_ctx::BlasHost & H = c->blas[blas_id];
    if (!H.normals.set) { c->err = "rtx_blas_pseudonormals: no topology set since the alloc (rtx_set_blas_topology)"; return RTX_ERR_STATE; }
    if (!H.refit.bound) { c->err = "rtx_blas_pseudonormals: no vertices bound to the id (rtx_bind_blas_vertices, or rtx_alloc_blas)"; return RTX_ERR_STATE; }
    if (H.normals.dev.vertex_count != H.refit.vertex_count) {
        c->err = "rtx_blas_pseudonormals: the topology's vertex_count (" + std::to_string(H.normals.dev.vertex_count) + ") differs from the bound one (" + std::to_string(H.refit.vertex_count) + ")";
        return RTX_ERR_INVALID_ARG;
    }
    hipSetDevice(c->cfg.device);
    const size_t T = (size_t)H.normals.dev.tri_count, V = (size_t)H.normals.dev.vertex_count, slots = (size_t)c->h_blas[blas_id].tri_count;
    if (!H.side.allocated) {
        rtx_ctx::BlasSide N;
        // [face records][vertex pseudonormals][edge pseudonormals], every part 256-byte aligned
        const size_t len[3] = { T * RTX_SIDE_RECORD * 16, V * 16, (slots ? slots : 1) * 3 * 16 };
        size_t off[3];
        if (int rc = ensure(c, N.block, aligned_parts(len, off, 3))) return rc;
        char * const bb = (char *)N.block.p;
        memset(&N.dev, 0, sizeof(N.dev));
        N.dev.record = (float4 *)(bb + off[0]); N.dev.vert_pn = (float4 *)(bb + off[1]); N.dev.edge_pn = (float4 *)(bb + off[2]);
        N.dev.indices = H.normals.dev.indices; N.dev.keys = H.normals.dev.keys; N.dev.offset = H.normals.dev.offset;
        N.dev.slot_vertices = H.refit.dev.slot_vertices;
        N.dev.tri_count = (int32_t)T; N.dev.vertex_count = (int32_t)V; N.dev.slots = (int32_t)slots;
        N.allocated = true;
        if (c->h_side.size() < c->h_blas.size()) { DevSideBlas none; memset(&none, 0, sizeof(none)); c->h_side.resize(c->h_blas.size(), none); }
        HIP_OK(c, hipStreamSynchronize(c->stream));
        H.side = std::move(N);
        DevSideBlas & e = c->h_side[blas_id];
        e.vert_pn = H.side.dev.vert_pn; e.edge_pn = H.side.dev.edge_pn; e.slot_vertices = H.side.dev.slot_vertices; e.vertex_count = (int32_t)V; e.pad = 0;
        c->side_dirty = true;
    }
    DevSide & d = H.side.dev;
    d.positions = (const float *)positions_dev;
    launch_timed(c, "k_side_faces", c->stream, [&] { hipLaunchKernelGGL(k_side_faces, dim3(((uint32_t)d.tri_count + RTX_SIDE_BLOCK - 1) / RTX_SIDE_BLOCK), dim3(RTX_SIDE_BLOCK), 0, c->stream, d); });
    launch_timed(c, "k_side_vertices", c->stream, [&] { hipLaunchKernelGGL(k_side_vertices, dim3(((uint32_t)d.vertex_count + RTX_SIDE_BLOCK - 1) / RTX_SIDE_BLOCK), dim3(RTX_SIDE_BLOCK), 0, c->stream, d); });
    if (d.slots) launch_timed(c, "k_side_edges", c->stream, [&] { hipLaunchKernelGGL(k_side_edges, dim3((3u * (uint32_t)d.slots + RTX_SIDE_BLOCK - 1) / RTX_SIDE_BLOCK), dim3(RTX_SIDE_BLOCK), 0, c->stream, d); });
    HIP_OK(c, hipGetLastError());
    return RTX_OK;
}

extern "C" int rtx_read_blas_pseudonormals(rtx_ctx * c, int32_t blas_id, float * vert_out, float * edge_out) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (blas_id < 0 || blas_id >= (1 << 20) || (!vert_out && !edge_out)) { c->err = "rtx_read_blas_pseudonormals: bad id or nothing to read into"; return RTX_ERR_INVALID_ARG; }
    if ((size_t)blas_id >= c->blas.size() || !c->blas[blas_id].side.allocated) { c->err = "rtx_read_blas_pseudonormals: no pseudonormal tables under that id (rtx_blas_pseudonormals)"; return RTX_ERR_STATE; }
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    const DevSide & d = c->blas[blas_id].side.dev;
    if (vert_out) HIP_OK(c, hipMemcpy(vert_out, d.vert_pn, (size_t)d.vertex_count * 16, hipMemcpyDeviceToHost));
    if (edge_out && d.slots) HIP_OK(c, hipMemcpy(edge_out, d.edge_pn, (size_t)d.slots * 3 * 16, hipMemcpyDeviceToHost));
    return RTX_OK;
}

extern "C" int rtx_read_blas(rtx_ctx * c, int32_t blas_id, rtx_bvh_node * nodes, rtx_triangle_hot * hot, rtx_triangle_cold * cold) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (blas_id < 0 || blas_id >= (1 << 20)) { c->err = "rtx_read_blas: bad id"; return RTX_ERR_INVALID_ARG; }
    if ((size_t)blas_id >= c->h_blas.size() || !c->h_blas[blas_id].nodes) { c->err = "rtx_read_blas: no BLAS uploaded under that id"; return RTX_ERR_STATE; }
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    const DevBlas & B = c->h_blas[blas_id];
    if (nodes) if (int rc = read_lane_nodes(c, B.nodes, B.node_count, nodes)) return rc;
    if (hot && B.tri_count) {
        std::vector<float4> th((size_t)RTX_TRI_STRIDE * B.tri_count);
        HIP_OK(c, hipMemcpy(th.data(), B.tri_hot, th.size() * 16, hipMemcpyDeviceToHost));
        for (int i = 0; i < B.tri_count; i++) {
            const float4 * t = &th[(size_t)RTX_TRI_STRIDE * i];
            hot[i].position_0[0] = t[0].x; hot[i].position_0[1] = t[0].y; hot[i].position_0[2] = t[0].z;
            hot[i].position_edge_1[0] = t[1].x; hot[i].position_edge_1[1] = t[1].y; hot[i].position_edge_1[2] = t[1].z;
            hot[i].position_edge_2[0] = t[2].x; hot[i].position_edge_2[1] = t[2].y; hot[i].position_edge_2[2] = t[2].z;
        }
    }
    if (cold && B.tri_count) HIP_OK(c, hipMemcpy(cold, B.tri_cold, (size_t)B.tri_count * sizeof(rtx_triangle_cold), hipMemcpyDeviceToHost));
    return RTX_OK;
}

// ---- device-side texture and sky update (include/rtx.h: rtx_alloc_texture / rtx_update_texture / rtx_read_texture / rtx_update_sky;
// kernels in rtx_texmip.h) ---------------------------------------------------------------------------------------------------------------
// Everything the host decides about a chain — its shape, the passes that rewrite it — follows from (width, height, mipmapped, P) and is
// decided at the alloc.  An update is then queued like a refit: it writes the texels in place, touches no pointer and reads nothing back.
extern "C" int rtx_alloc_texture(rtx_ctx * c, int32_t texture_id, int32_t width, int32_t height, int32_t mipmapped) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (texture_id < 0 || texture_id >= 4096 || width < 1 || height < 1) { c->err = "rtx_alloc_texture: id outside [0, 4096) or an empty side"; return RTX_ERR_INVALID_ARG; }
    rtx_texture_desc desc; int64_t texel_count = 0;
    if (rtxt::chain_shape(width, height, mipmapped, &desc, &texel_count)) { c->err = "rtx_alloc_texture: more than RTX_MAX_MIP_LEVELS levels, or more texels than the int32_t offsets hold"; return RTX_ERR_LIMIT; }
    hipSetDevice(c->cfg.device);
    if (!c->d_srgb_lut.p) {
        float lut[256];                                                     // colour_unpack + Math::gamma_to_linear as rtxh_texture_load evaluates them (host/rtx_image.cpp), host libm
        for (int b = 0; b < 256; b++) {
            const float x = float(b) * 0.00392156862f;
            lut[b] = x <= 0.0f ? 0.0f : x >= 1.0f ? 1.0f : x < 0.04045f ? x / 12.92f : powf((x + 0.055f) / 1.055f, 2.4f);
        }
        DevBuf t;
        if (int rc = upload(c, t, lut, sizeof(lut))) return rc;
        c->d_srgb_lut = std::move(t);
    }
    DevBuf d;
    if (int rc = ensure(c, d, (size_t)texel_count * 16)) return rc;
    HIP_OK(c, hipMemsetAsync(d.p, 0, (size_t)texel_count * 16, c->stream));      // ordered before every update and render call; rtx_set_stream waits for it
    rtx_ctx::TexUpdate U;
    U.allocated = true;
    U.plan = rtxt::plan_passes(width, height, desc.mip_levels, c->knobs.tex_pass_levels);
    return commit_texture(c, texture_id, desc, d, U);
}

extern "C" int rtx_update_texture(rtx_ctx * c, int32_t texture_id, const void * texels_dev, int32_t format) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!texels_dev || (format != RTX_TEXELS_RGB_F32 && format != RTX_TEXELS_RGBA8_SRGB) || (format == RTX_TEXELS_RGB_F32 && ((uintptr_t)texels_dev & 3))) {
        c->err = "rtx_update_texture: null or misaligned texel pointer, or an unknown format"; return RTX_ERR_INVALID_ARG; }
    if (texture_id < 0 || (size_t)texture_id >= c->h_tex.size() || !c->h_tex[texture_id].texels || !c->tex_update[texture_id].allocated) {
        c->err = "rtx_update_texture: the id was not created by rtx_alloc_texture (or was uploaded again since)"; return RTX_ERR_STATE; }
    hipSetDevice(c->cfg.device);
    const rtxt::Plan & plan = c->tex_update[texture_id].plan;
    float4 * const chain = (float4 *)c->tex_texels[texture_id].p;
    const float * const lut = (const float *)c->d_srgb_lut.p;
    for (int k = 0; k < plan.count; k++) {
        const rtxt::Pass & p = plan.pass[k];
        const dim3 grid((unsigned)(p.tiles_x * p.tiles_y)), block(rtxt::BLOCK);
        if (k > 0) launch_timed(c, "k_texmip_chain", c->stream, [&] { hipLaunchKernelGGL(k_texmip<TEXMIP_CHAIN>, grid, block, 0, c->stream, p, (const void *)nullptr, chain, lut); });
        else if (format == RTX_TEXELS_RGB_F32) launch_timed(c, "k_texmip_rgb_f32", c->stream, [&] { hipLaunchKernelGGL(k_texmip<TEXMIP_RGB_F32>, grid, block, 0, c->stream, p, texels_dev, chain, lut); });
        else launch_timed(c, "k_texmip_rgba8", c->stream, [&] { hipLaunchKernelGGL(k_texmip<TEXMIP_RGBA8_SRGB>, grid, block, 0, c->stream, p, texels_dev, chain, lut); });
    }
    HIP_OK(c, hipGetLastError());
    return RTX_OK;
}

extern "C" int rtx_read_texture(rtx_ctx * c, int32_t texture_id, rtx_texture_desc * desc, float * texels_rgb, int64_t capacity_texels) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (texture_id < 0 || texture_id >= 4096) { c->err = "rtx_read_texture: bad id"; return RTX_ERR_INVALID_ARG; }
    if ((size_t)texture_id >= c->h_tex.size() || !c->h_tex[texture_id].texels) { c->err = "rtx_read_texture: no texture under that id"; return RTX_ERR_STATE; }
    const DevTexture & T = c->h_tex[texture_id];
    int64_t count = 0;                         // the end of the level that ends last: a caller-made chain need not be laid out in level order
    for (int l = 0; l < T.desc.mip_levels; l++) {
        const int64_t end = (int64_t)T.desc.mip_offsets[l] + (int64_t)(T.desc.width >> l) * (T.desc.height >> l);
        if (end > count) count = end;
    }
    if (texels_rgb && capacity_texels < count) { c->err = "rtx_read_texture: capacity_texels is smaller than the chain"; return RTX_ERR_INVALID_ARG; }
    if (desc) *desc = T.desc;
    if (!texels_rgb) return RTX_OK;
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    std::vector<float4> padded((size_t)count);
    HIP_OK(c, hipMemcpy(padded.data(), T.texels, (size_t)count * 16, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < count; i++) { texels_rgb[3 * i] = padded[(size_t)i].x; texels_rgb[3 * i + 1] = padded[(size_t)i].y; texels_rgb[3 * i + 2] = padded[(size_t)i].z; }
    return RTX_OK;
}

extern "C" int rtx_update_sky(rtx_ctx * c, const void * texels_dev, int32_t size) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!texels_dev || ((uintptr_t)texels_dev & 3)) { c->err = "rtx_update_sky: null or misaligned texel pointer"; return RTX_ERR_INVALID_ARG; }
    if (!c->sky_uploaded) { c->err = "rtx_update_sky: no probe to copy over (rtx_upload_sky)"; return RTX_ERR_STATE; }
    if (size != c->sky_size) { c->err = "rtx_update_sky: size differs from the uploaded one"; return RTX_ERR_INVALID_ARG; }
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipMemcpyAsync(c->d_sky.p, texels_dev, (size_t)size * size * 12, hipMemcpyDeviceToDevice, c->stream));      // the padding texel behind stays zero
    return RTX_OK;
}

// The layouts derived from the lane layout, as the kernels read them now: plain copies after a wait for the stream, nothing is launched and
// nothing of the context changes.  blas_id -1: the TLAS of the frame in the packet layout.
extern "C" int rtx_debug_read_layouts(rtx_ctx * c, int32_t blas_id, int32_t * info8, float * pk_nodes, float * pk4_nodes, float * pk4c_nodes,
                                      float * planes_x, float * planes_y, float * planes_z) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (blas_id < -1 || blas_id >= (1 << 20)) { c->err = "rtx_debug_read_layouts: bad id"; return RTX_ERR_INVALID_ARG; }
    int32_t info[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (blas_id == -1) {
        if (!c->frame_set) { c->err = "rtx_debug_read_layouts before rtx_set_frame"; return RTX_ERR_STATE; }
        hipSetDevice(c->cfg.device);
        HIP_OK(c, hipStreamSynchronize(c->stream));
        const DevScene & s = c->scene;
        info[0] = s.tlas_node_count;
        if (info8) memcpy(info8, info, sizeof(info));
        if (pk_nodes && s.tlas_node_count) HIP_OK(c, hipMemcpy(pk_nodes, s.pk_tlas_nodes, (size_t)s.tlas_node_count * 32, hipMemcpyDeviceToHost));
        return RTX_OK;
    }
    if ((size_t)blas_id >= c->h_blas.size() || !c->h_blas[blas_id].nodes) { c->err = "rtx_debug_read_layouts: no BLAS uploaded under that id"; return RTX_ERR_STATE; }
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    const DevBlas & B = c->h_blas[blas_id];
    info[0] = B.node_count; info[1] = B.pk4_nodes ? 1 : 0; info[2] = B.pk4c_nodes ? 1 : 0;
    for (int a = 0; a < 3; a++) info[3 + a] = B.plane_count[a];
    if (info8) memcpy(info8, info, sizeof(info));
    const size_t wide_bytes = ((size_t)4 * B.node_count + 8) * 16;
    if (pk_nodes) HIP_OK(c, hipMemcpy(pk_nodes, B.pk_nodes, (size_t)B.node_count * 32, hipMemcpyDeviceToHost));
    if (pk4_nodes && B.pk4_nodes) HIP_OK(c, hipMemcpy(pk4_nodes, B.pk4_nodes, wide_bytes, hipMemcpyDeviceToHost));
    if (pk4c_nodes && B.pk4c_nodes) HIP_OK(c, hipMemcpy(pk4c_nodes, B.pk4c_nodes, wide_bytes, hipMemcpyDeviceToHost));
    float * const planes[3] = { planes_x, planes_y, planes_z };
    for (int a = 0; a < 3; a++)
        if (planes[a] && B.plane_count[a]) HIP_OK(c, hipMemcpy(planes[a], B.planes[a], (size_t)B.plane_count[a] * 4, hipMemcpyDeviceToHost));
    return RTX_OK;
}

// The three stack figures plan_stack_limits reads, from the uploaded trees: what render calls and ray queries both decide lane / pk_closest by
static StackFigures stack_figures(const rtx_ctx * c) {
    StackFigures s = { false, c->tlas_inner_depth < 0 ? 0 : c->tlas_inner_depth + 1, 0, 0 };
    for (size_t b = 0; b < c->h_blas.size(); b++) {
        if (!c->h_blas[b].nodes) continue;
        if (!c->blas[b].packet_ok) s.unfit_mesh = true;
        const int depth = c->blas[b].inner_depth + 2;
        const int any = c->h_blas[b].pk4_nodes ? c->h_blas[b].pk4_need : depth;
        if (any > s.blas_any) s.blas_any = any;
        if (2 * depth > s.blas_shared) s.blas_shared = 2 * depth;
    }
    return s;
}

static int render_tiles_impl(rtx_ctx * c, int32_t first_tile, int32_t tile_stride, int32_t tile_count, uint32_t flags, uint32_t * tile_major, int views = RTX_CAM_TILES);
static int aov_targets_of_call(rtx_ctx * c, int64_t pixels, DevAov & out);

extern "C" int rtx_render_tiles(rtx_ctx * c, int32_t first_tile, int32_t tile_stride, int32_t tile_count, uint32_t flags) {
    return render_tiles_impl(c, first_tile, tile_stride, tile_count, flags, nullptr);
}

// ---- a render call: check -> plan -> allocate -> graph key -> run.  The decisions are plan_render's (rtx_plan.h); this is the only place
// that collects what they read from the context
static PlanInputs gather_plan_inputs(const rtx_ctx * c, uint32_t flags, int views, int tile_count, int batch_tiles, bool tile_major) {
    PlanInputs in; memset(&in, 0, sizeof(in));
    in.flags = flags; in.views = views; in.tile_count = tile_count; in.batch_tiles = batch_tiles; in.tile_major = tile_major; in.timing = c->timing;
    in.knobs = c->knobs;
    in.instance_count = c->scene.instance_count; in.light_count = c->scene.light_count; in.bounces = c->cfg.bounces; in.heatmap = c->scene.heatmap != 0;
    in.can_spawn = plan_can_spawn(c->h_materials.data(), c->h_materials.size());
    in.all_wide = all_meshes_wide(c);
    in.stack = stack_figures(c);
    in.n_cu = c->n_cu; in.pk_blocks_closest = c->pk_blocks_closest; in.pk_blocks_any = c->pk_blocks_any;
    in.lone = c->frame_lone.lone; in.copy_class = c->frame_lone.copy_class;
    return in;
}

// What the plan wants of the context, before anything of the call is queued and before any capture begins: the stats partials, the split
// walk's item buffer (the buffer only ever grows; if it cannot be had the plan loses its split, see plan_drop_split), the LPT buffers, and
// every stream and event the launches will use
static int alloc_for_plan(rtx_ctx * c, RenderPlan & plan) {
    if (int rc = ensure(c, c->d_stats_partial, (size_t)(RTX_MAX_LEVELS + 1) * plan.stats_stride * 4 * sizeof(uint32_t))) return rc;
    c->q.pk_items = nullptr; c->q.pk_item_count = nullptr; c->q.pk_item_cap = 0;
    if (plan.split) {
        const size_t chunks = (size_t)c->pk_blocks_any * (RTX_PK_BLOCK / RTX_WAVE);
        int cap = plan.item_cap;
        if (cap <= c->item_cap_alloc && c->d_pk_items.p && !c->knobs.fail_item_alloc) cap = c->item_cap_alloc;      // the buffer is there already
        else {
            c->item_cap_alloc = 0;
            const size_t bytes = c->knobs.fail_item_alloc ? ((size_t)1 << 46) : chunks * (size_t)cap * 48;
            if (ensure(c, c->d_pk_items, bytes) == 0 && ensure(c, c->d_pk_item_count, chunks * 4) == 0) c->item_cap_alloc = cap;
            else { (void)hipGetLastError(); c->err.clear(); cap = 0; }       // fall back to the in-kernel per-lane phase
        }
        if (cap >= 64) { c->q.pk_items = (uint4 *)c->d_pk_items.p; c->q.pk_item_count = (uint32_t *)c->d_pk_item_count.p; c->q.pk_item_cap = cap; }
        else plan_drop_split(plan);
    }
    c->q.pk_cost = nullptr; c->q.pk_lpt_order = nullptr;
    if (plan.lpt) {
        if (int rc = ensure(c, c->d_pk_cost, (size_t)plan.lpt_n * 4)) return rc;
        if (int rc = ensure(c, c->d_pk_order, (size_t)plan.lpt_n * 4)) return rc;
        if (!c->order_stream) HIP_OK(c, hipStreamCreateWithFlags(&c->order_stream, hipStreamNonBlocking));
        if (!c->ev_cost) HIP_OK(c, hipEventCreateWithFlags(&c->ev_cost, hipEventDisableTiming));
        if (!c->ev_order) HIP_OK(c, hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming));
    }
    if (plan.overlap && !c->any_stream) HIP_OK(c, hipStreamCreateWithFlags(&c->any_stream, hipStreamNonBlocking));
    return RTX_OK;
}

// RTX_PK_LPT, before the launches: the order of the previous call is used only if that call covered the same packets; either way the main
// stream waits for the previous call's sort, which still reads the cost buffer.  (An LPT call is never a graph call.)
static int lpt_begin(rtx_ctx * c, const RenderPlan & plan, int32_t first_tile, int32_t tile_stride, int32_t tile_count) {
    if (!plan.lpt) { c->lpt_valid = false; return RTX_OK; }
    const int32_t key[5] = { first_tile, tile_stride, tile_count, plan.levels, plan.views };      // view calls and ray calls have key spaces of their own: packets over views x tiles
    const bool use_order = c->lpt_valid && memcmp(key, c->lpt_key, sizeof(key)) == 0;
    memcpy(c->lpt_key, key, sizeof(key));
    c->q.pk_cost = (uint32_t *)c->d_pk_cost.p;
    if (use_order) c->q.pk_lpt_order = (const uint32_t *)c->d_pk_order.p;
    if (c->lpt_valid) HIP_OK(c, hipStreamWaitEvent(c->stream, c->ev_order, 0));
    return RTX_OK;
}

// the launches that generate primary rays or read the camera take the VIEWS / RAYS instantiation of their kernel in a view / ray call
template <typename F>
static void with_views(int views, F && launch) {
    if (views == RTX_CAM_RAYS) launch(std::integral_constant<int, RTX_CAM_RAYS>()); else if (views) launch(std::integral_constant<int, RTX_CAM_VIEWS>()); else launch(std::integral_constant<int, RTX_CAM_TILES>());
}

static void launch_closest(rtx_ctx * c, const RenderPlan & plan, const DevScene & sc, const DevQueues & q, int level) {
    const int kernel = plan.closest[level];
    const bool fused = kernel == CLOSEST_PACKET_FUSED || kernel == CLOSEST_PACKET_FUSED_CULL;
    launch_timed(c, fused ? "k_trace_closest_shade" : "k_trace_closest", c->stream, [&] { with_views(plan.views, [&](auto V) { constexpr int VW = decltype(V)::value;
        const dim3 plain(c->trace_blocks_count), lane(c->trace_blocks_closest), tb(RTX_TRACE_BLOCK), pk(c->pk_blocks_closest), pb(RTX_PK_BLOCK);
        switch (kernel) {
        case CLOSEST_PLAIN_COUNT:       hipLaunchKernelGGL((k_trace<false, true, VW>),  plain, tb, 0, c->stream, sc, q, level); break;
        case CLOSEST_PLAIN:             hipLaunchKernelGGL((k_trace<false, false, VW>), plain, tb, 0, c->stream, sc, q, level); break;
        case CLOSEST_LANE:              hipLaunchKernelGGL((k_trace_fast<false, VW>),   lane, tb, 0, c->stream, sc, q, level, level); break;
        case CLOSEST_PACKET_STATS:      hipLaunchKernelGGL((k_packet<false, true, false, false, false, VW>),  pk, pb, 0, c->stream, sc, q, level, level); break;
        case CLOSEST_PACKET_FUSED_CULL: hipLaunchKernelGGL((k_packet<false, false, false, true, true, VW>),   pk, pb, 0, c->stream, sc, q, level, level); break;
        case CLOSEST_PACKET_FUSED:      hipLaunchKernelGGL((k_packet<false, false, false, true, false, VW>),  pk, pb, 0, c->stream, sc, q, level, level); break;
        default:                        hipLaunchKernelGGL((k_packet<false, false, false, false, false, VW>), pk, pb, 0, c->stream, sc, q, level, level); break;
        }
    }); });
}

static void launch_shade(rtx_ctx * c, const RenderPlan & plan, const DevScene & sc, const DevQueues & q, const DevAov & aov_t, int level) {
    if (plan.shade[level] == SHADE_NONE) return;
    launch_timed(c, "k_shade", c->stream, [&] { with_views(plan.views, [&](auto V) { constexpr int VW = decltype(V)::value;
        const dim3 g(plan_level_blocks(q.primary_slots, level, plan.shade_blocks)), b(RTX_SHADE_BLOCK);
        switch (plan.shade[level]) {
        case SHADE_AOV_COUNT: hipLaunchKernelGGL((k_shade<true, false, VW, true, DevAov>),  g, b, 0, c->stream, sc, q, level, aov_t); break;
        case SHADE_AOV_CULL:  hipLaunchKernelGGL((k_shade<false, true, VW, true, DevAov>),  g, b, 0, c->stream, sc, q, level, aov_t); break;
        case SHADE_AOV:       hipLaunchKernelGGL((k_shade<false, false, VW, true, DevAov>), g, b, 0, c->stream, sc, q, level, aov_t); break;
        case SHADE_COUNT:     hipLaunchKernelGGL((k_shade<true, false, VW>),  g, b, 0, c->stream, sc, q, level); break;
        case SHADE_CULL:      hipLaunchKernelGGL((k_shade<false, true, VW>),  g, b, 0, c->stream, sc, q, level); break;
        default:              hipLaunchKernelGGL((k_shade<false, false, VW>), g, b, 0, c->stream, sc, q, level); break;
        }
    }); });
}

// one entry of the shadow-ray schedule; split walk (RTX_PK_SPLIT): q.pk_items / q.pk_item_cap were sized for the call's largest batch
static void launch_any(rtx_ctx * c, const AnyLaunch & a, const DevScene & sc, const DevQueues & q) {
    const hipStream_t st = a.stream ? c->any_stream : c->stream;
    const dim3 plain(c->trace_blocks_count), lane(c->trace_blocks_any), tb(RTX_TRACE_BLOCK), pk(c->pk_blocks_any), pb(RTX_PK_BLOCK);
    launch_timed(c, "k_trace_any", st, [&] {
        switch (a.kernel) {
        case ANY_PLAIN_COUNT:   hipLaunchKernelGGL((k_trace<true, true>),   plain, tb, 0, st, sc, q, a.lo); break;
        case ANY_PLAIN:         hipLaunchKernelGGL((k_trace<true, false>),  plain, tb, 0, st, sc, q, a.lo); break;
        case ANY_LANE:          hipLaunchKernelGGL((k_trace_fast<true>),    lane, tb, 0, st, sc, q, a.lo, a.hi); break;
        case ANY_PACKET_STATS:  hipLaunchKernelGGL((k_packet<true, true>),  pk, pb, 0, st, sc, q, a.lo, a.hi); break;
        case ANY_PACKET_SPLIT:  hipLaunchKernelGGL((k_packet<true, false, true>), pk, pb, 0, st, sc, q, a.lo, a.hi); break;
        default:                hipLaunchKernelGGL((k_packet<true, false>), pk, pb, 0, st, sc, q, a.lo, a.hi); break;
        }
    });
    if (a.items) launch_timed(c, "k_trace_items", st, [&] { hipLaunchKernelGGL(k_items, dim3(c->item_blocks), dim3(RTX_ITEM_BLOCK), 0, st, sc, q, c->pk_blocks_any * (RTX_PK_BLOCK / RTX_WAVE), a.lo); });
}

// Executes the plan for one batch of tiles (q: the batch's queues).  Main stream: closest(d) -> shade(d) for d = 0 .. levels-1, the shadow-ray
// schedule's entries after the level they name — on the shadow-ray stream behind an event where the plan overlaps them — then k_resolve from
// the deepest level up.
static int run_batch(rtx_ctx * c, const RenderPlan & plan, const DevScene & sc, const DevQueues & q, const DevAov & aov_t, bool first_batch) {
    begin_batch(c, q.counters, q.pk_heads, (uint32_t)q.primary_slots, plan.plain != 0, first_batch);
    if (plan.heatmap) {
        launch_closest(c, plan, sc, q, 0);
        launch_timed(c, "k_heatmap", c->stream, [&] { with_views(plan.views, [&](auto V) { if constexpr (decltype(V)::value != RTX_CAM_RAYS) hipLaunchKernelGGL((k_heatmap<decltype(V)::value>), dim3(plan.stream_blocks), dim3(256), 0, c->stream, sc, q); }); });
        return RTX_OK;
    }
    int next_any = 0;
    for (int level = 0; level < plan.levels; level++) {
        launch_closest(c, plan, sc, q, level);
        if (plan.lpt && level == 0) {
            HIP_OK(c, hipEventRecord(c->ev_cost, c->stream)); HIP_OK(c, hipStreamWaitEvent(c->order_stream, c->ev_cost, 0));
            hipLaunchKernelGGL(k_packet_order, dim3(1), dim3(1024), 0, c->order_stream, (const uint32_t *)c->d_pk_cost.p, (uint32_t *)c->d_pk_order.p, plan.lpt_n);
            HIP_OK(c, hipEventRecord(c->ev_order, c->order_stream));
            c->lpt_valid = true;
        }
        launch_shade(c, plan, sc, q, aov_t, level);
        bool joined = false;      // the shadow-ray stream waits for this level's k_shade once
        for (; next_any < plan.n_any && plan.any[next_any].after_level == level; next_any++) {
            if (plan.any[next_any].stream && !joined) {
                const hipEvent_t ev = level == 0 ? c->ev_shade0 : c->ev_shade_last;
                HIP_OK(c, hipEventRecord(ev, c->stream)); HIP_OK(c, hipStreamWaitEvent(c->any_stream, ev, 0));
                joined = true;
            }
            launch_any(c, plan.any[next_any], sc, q);
        }
    }
    if (plan.overlap) { HIP_OK(c, hipEventRecord(c->ev_any_done, c->any_stream)); HIP_OK(c, hipStreamWaitEvent(c->stream, c->ev_any_done, 0)); }
    for (int level = plan.levels - 1; level >= 0; level--)
        launch_timed(c, "k_resolve", c->stream, [&] { with_views(plan.views, [&](auto V) {
            hipLaunchKernelGGL((k_resolve<decltype(V)::value>), dim3(plan_level_blocks(q.primary_slots, level, plan.stream_blocks) * (256 / plan.resolve_block)), dim3(plan.resolve_block), 0, c->stream, sc, q, level); }); });
    return RTX_OK;
}

// hipGraph replay: the kernel arguments of a call are functions of (scene, queues, plan, tile range, AOV targets); while those bytes stay the
// same the captured graph IS the call.  The plan holds the flags, the views mode and every decision drawn from knobs, tree depths and scene
// counts, so nothing a launch depends on is missing from the key.  A view call's view range is its tile range (first_tile = first_view * tiles
// per view) and its cameras are read from device memory at replay; a ray call carries the address of its rays in the queues: a rebind is a new
// key, new values in the same buffer are read at replay.  The AOV targets are zero for a call without RTX_RENDER_AOV: a rebind is a new key.
static std::vector<unsigned char> graph_key_of(const rtx_ctx * c, const RenderPlan & plan, int32_t first_tile, int32_t tile_stride, int32_t tile_count, const uint32_t * tile_major, const DevAov & aov_t) {
    const int32_t range[3] = { first_tile, tile_stride, tile_count };
    const struct { const void * p; size_t n; } parts[] = { { &c->scene, sizeof(DevScene) }, { &c->q, sizeof(DevQueues) }, { &plan, sizeof(plan) }, { range, sizeof(range) }, { &tile_major, sizeof(tile_major) }, { &aov_t, sizeof(aov_t) } };
    std::vector<unsigned char> key;
    for (const auto & part : parts) key.insert(key.end(), (const unsigned char *)part.p, (const unsigned char *)part.p + part.n);
    return key;
}

// the end of a capture window, reached on every path out of it: the capture is ended first; on a failure (rc: of the launches) the graph is
// discarded and graph_key cleared, so the next identical call starts over
static int graph_finish(rtx_ctx * c, int rc) {
    hipGraph_t g = nullptr;
    const hipError_t ce = hipStreamEndCapture(c->stream, &g);
    hipError_t ie = hipSuccess;
    if (!rc && ce == hipSuccess && g) ie = hipGraphInstantiate(&c->graph_exec, g, nullptr, nullptr, 0);
    if (g) hipGraphDestroy(g);
    if (rc || ce != hipSuccess || !g || ie != hipSuccess) {
        hipGetLastError(); c->graph_exec = nullptr; c->graph_key.clear();
        if (!rc) c->err = (ce != hipSuccess || !g) ? "hipGraph capture failed" : "hipGraphInstantiate failed";
        return rc ? rc : RTX_ERR_HIP;
    }
    HIP_OK(c, hipGraphLaunch(c->graph_exec, c->stream));
    return RTX_OK;
}

// tile_major != nullptr: the packed level-0 pixels of the i-th rendered tile go to tile_major[i * 1024 ...] (slot order) instead of the framebuffer.
// views (rtx_render_views): the tiles are virtual tiles over views x tiles of the set views (range checked by the caller), the kernels are the
// VIEWS instantiations and level 0 writes the view framebuffer.  RTX_CAM_RAYS (rtx_render_rays): the same over the ray views, with the rays
// instantiations, which read their primary rays from the current ray buffer
static int render_tiles_impl(rtx_ctx * c, int32_t first_tile, int32_t tile_stride, int32_t tile_count, uint32_t flags, uint32_t * tile_major, int views) {
    if (!c || first_tile < 0 || tile_stride < 1 || tile_count < 0) return RTX_ERR_INVALID_ARG;
    if (!c->frame_set) { c->err = "rtx_render_tiles before rtx_set_frame"; return RTX_ERR_STATE; }
    if (int bad = validate_references(c)) return bad;
    if (!views && tile_count > 0 && first_tile + (int64_t)(tile_count - 1) * tile_stride >= (int64_t)frame_tiles(c)) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    // RTX_RENDER_AOV: level 0 takes k_shade<.., AOV = true> with the bound channels' targets; the call's pixel range is the frame, or its views
    DevAov aov_t = {};
    if (flags & RTX_RENDER_AOV) {
        if (tile_major) { c->err = "RTX_RENDER_AOV is not supported on the rtx_group_* path"; return RTX_ERR_INVALID_ARG; }
        if (c->scene.heatmap) { c->err = "RTX_RENDER_AOV in heat-map mode (a heat-map frame has no shading)"; return RTX_ERR_STATE; }
        if (!c->aov_channels) { c->err = "RTX_RENDER_AOV without channels bound by rtx_bind_aovs"; return RTX_ERR_STATE; }
        const int64_t frame_px = (int64_t)c->cfg.width * c->cfg.height;
        const int64_t pixels = views ? ((int64_t)first_tile + tile_count) / (int64_t)frame_tiles(c) * frame_px : frame_px;
        if (int arc = aov_targets_of_call(c, pixels, aov_t)) return arc;
    }
    c->serial = (flags & RTX_RENDER_SERIAL) != 0;

    // stats of this call are reset by the first k_begin_batch (WorkerThread.cpp:120 zeroes them per frame)
    if (tile_count == 0) { begin_batch(c, (DevCounters *)c->d_counters.p, (uint32_t *)c->d_pk_heads.p, 0u, false, true); c->stats_pending = true; return RTX_OK; }

    int batch_tiles = 0;
    plan_batch(c, tile_count, batch_tiles);
    if (int rc = alloc_queues(c, batch_tiles)) return rc;
    if (views) {
        // one field for both: the cameras of a view call, or (cast) the rtx_ray records of a ray call, read by the instantiation that knows which
        c->q.views = views == RTX_CAM_RAYS ? (const rtx_camera *)(c->ext_rays ? c->ext_rays : c->d_rays.p) : (const rtx_camera *)c->d_views.p;
        c->q.fb_rgb = (float *)(c->ext_vrgb ? c->ext_vrgb : c->d_vfb_rgb.p);
        c->q.fb_packed = (uint32_t *)(c->ext_vpacked ? c->ext_vpacked : c->d_vfb_packed.p);
    }
    RenderPlan plan = plan_render(gather_plan_inputs(c, flags, views, tile_count, batch_tiles, tile_major != nullptr));
    if (int rc = alloc_for_plan(c, plan)) return rc;
    if (int rc = lpt_begin(c, plan, first_tile, tile_stride, tile_count)) return rc;

    bool capturing = false;
    if (plan.graph_eligible) {
        std::vector<unsigned char> key = graph_key_of(c, plan, first_tile, tile_stride, tile_count, tile_major, aov_t);
        if (c->graph_exec && key == c->graph_key) {
            HIP_OK(c, hipGraphLaunch(c->graph_exec, c->stream));
            c->stats_pending = true;
            return RTX_OK;
        }
        if (c->graph_exec) { hipGraphExecDestroy(c->graph_exec); c->graph_exec = nullptr; }
        if (c->graph_warm == key) {           // second identical call: capture (the first one ran eagerly: lazy allocations, stream creation)
            if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) { capturing = true; c->graph_key.swap(key); }
            else hipGetLastError();
        } else c->graph_warm.swap(key);
    }
    int rc = RTX_OK;
    for (int done = 0; done < tile_count && !rc; done += batch_tiles) {
        const int n = (tile_count - done) < batch_tiles ? (tile_count - done) : batch_tiles;
        DevQueues q = c->q;
        if (plan.pk_closest) q.pk_defer_t0_closest = q.pk_defer_t0_primary = q.pk_defer_t0;
        q.first_tile = first_tile + done * tile_stride; q.tile_stride = tile_stride; q.tile_count = n; q.primary_slots = n * 1024;
        q.tm_packed = tile_major; q.tm_base = done * 1024;
        q.cull = plan.cull;
        q.stats_partial = (uint32_t *)c->d_stats_partial.p; q.stats_stride = plan.stats_stride;
        for (int d = 0; d <= RTX_MAX_LEVELS; d++) q.stats_n[d] = d < plan.levels && !plan.heatmap ? plan_stats_n(plan, q.primary_slots, d) : 0;
        rc = run_batch(c, plan, c->scene, q, aov_t, done == 0);
    }
    if (capturing) rc = graph_finish(c, rc);      // no path leaves a capture window open
    if (rc) return rc;
    HIP_OK(c, hipGetLastError());
    c->stats_pending = true;
    return RTX_OK;
}

extern "C" int rtx_synchronize(rtx_ctx * c) {
    if (!c) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

extern "C" int rtx_get_stats(rtx_ctx * c, rtx_stats * stats, rtx_work_counters * work) {
    if (!c) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    if (c->stats_pending) {
        DevCounters h;
        HIP_OK(c, hipMemcpyAsync(&h, c->d_counters.p, sizeof(DevCounters), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(c, hipStreamSynchronize(c->stream));
        c->stats_acc.num_primary_rays = h.stats[0]; c->stats_acc.num_shadow_rays = h.stats[1];
        c->stats_acc.num_reflection_rays = h.stats[2]; c->stats_acc.num_refraction_rays = h.stats[3];
        memset(&c->work_acc, 0, sizeof(c->work_acc));
        memcpy(&c->work_acc, h.work, sizeof(uint64_t) * 20);
        c->err_flags_acc = h.error_flags;
        c->stats_pending = false;
    }
    if (stats) *stats = c->stats_acc;
    if (work)  *work  = c->work_acc;
    if (c->err_flags_acc & ERR_STACK_OVERFLOW) { c->err = "BVH traversal stack overflow (BVH_TRAVERSAL_STACK_SIZE, Config.h:25)"; return RTX_ERR_LIMIT; }
    if (c->err_flags_acc & ERR_QUEUE_OVERFLOW) { c->err = "ray queue overflow"; return RTX_ERR_LIMIT; }
    return RTX_OK;
}

extern "C" int rtx_read_framebuffer(rtx_ctx * c, float * rgb_f32, uint32_t * packed_u32) {
    if (!c) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    const size_t px = (size_t)c->cfg.width * c->cfg.height;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    if (rgb_f32)    HIP_OK(c, hipMemcpy(rgb_f32, c->ext_rgb ? c->ext_rgb : c->d_fb_rgb.p, px * 12, hipMemcpyDeviceToHost));
    if (packed_u32) HIP_OK(c, hipMemcpy(packed_u32, c->ext_packed ? c->ext_packed : c->d_fb_packed.p, px * 4, hipMemcpyDeviceToHost));
    return RTX_OK;
}

// Window::draw_quad (Window.cpp:87-95): gamma 1/2.2 + optional FXAA over the packed frame, see rtx_present.h (parity unpinned vs GL)
extern "C" int rtx_present(rtx_ctx * c, int32_t enable_fxaa, uint32_t * display_u32, void ** display_dev) {
    if (!c) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    const size_t px = (size_t)c->cfg.width * c->cfg.height;
    int rc = ensure(c, c->d_display, px * 4);
    if (rc) return rc;
    if (!c->d_gamma.p) {
        rc = ensure(c, c->d_gamma, 256 * sizeof(float));
        if (rc) return rc;
        float lut[256];
        for (int i = 0; i < 256; i++) lut[i] = powf((float)i / 255.0f, 1.0f / 2.2f);         // pow(texel, vec3(1 / 2.2)), once per 8-bit value (host libm)
        HIP_OK(c, hipMemcpy(c->d_gamma.p, lut, sizeof(lut), hipMemcpyHostToDevice));
    }
    PresentArgs a;
    a.packed = (const uint32_t *)(c->ext_packed ? c->ext_packed : c->d_fb_packed.p);
    a.gamma_lut = (const float *)c->d_gamma.p; a.display = (uint32_t *)c->d_display.p;
    a.width = c->cfg.width; a.height = c->cfg.height; a.fxaa = enable_fxaa ? 1 : 0;
    hipLaunchKernelGGL(k_present, dim3((c->cfg.width + 15) / 16, (c->cfg.height + 15) / 16), dim3(256), 0, c->stream, a);   // after the frame, same stream
    HIP_OK(c, hipGetLastError());
    if (display_u32) {
        HIP_OK(c, hipStreamSynchronize(c->stream));
        HIP_OK(c, hipMemcpy(display_u32, c->d_display.p, px * 4, hipMemcpyDeviceToHost));
    }
    if (display_dev) *display_dev = c->d_display.p;
    return RTX_OK;
}

extern "C" int rtx_framebuffer_device_ptrs(rtx_ctx * c, void ** rgb_f32_dev, void ** packed_u32_dev) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (rgb_f32_dev) *rgb_f32_dev = c->ext_rgb ? c->ext_rgb : c->d_fb_rgb.p;
    if (packed_u32_dev) *packed_u32_dev = c->ext_packed ? c->ext_packed : c->d_fb_packed.p;
    return RTX_OK;
}

extern "C" int rtx_bind_framebuffer(rtx_ctx * c, void * rgb_f32_dev, void * packed_u32_dev) {
    if (!c || ((rgb_f32_dev == nullptr) != (packed_u32_dev == nullptr))) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    c->ext_rgb = rgb_f32_dev; c->ext_packed = packed_u32_dev;
    return RTX_OK;
}

extern "C" int rtx_set_stream(rtx_ctx * c, void * hip_stream) {
    if (!c) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return RTX_OK;
}

// ---- batches of views (include/rtx.h rtx_set_views ...) ------------------------------------------------------------------------------
// A view call is a render call over virtual tiles: view v's tile t is tile v * T + t, T = tiles per view (rtx_trace.h primary_pixel_v).
static int64_t view_pixel_count(const rtx_ctx * c, int64_t views) { return views * (int64_t)c->cfg.width * c->cfg.height; }
static int32_t current_ray_views(const rtx_ctx * c) { return c->ext_rays ? c->ext_ray_count : c->ray_count; }      // ray views of the bound buffer, else of the rays set

extern "C" int rtx_set_views(rtx_ctx * c, const rtx_camera * cameras, int32_t view_count) {
    if (!c || !cameras || view_count < 1 || view_count > RTX_MAX_VIEWS) return RTX_ERR_INVALID_ARG;
    if (view_pixel_count(c, view_count) >= (1ll << 31)) { c->err = "view_count * width * height must stay below 2^31 (pixel index of a ray record)"; return RTX_ERR_INVALID_ARG; }
    hipSetDevice(c->cfg.device);
    const size_t bytes = (size_t)view_count * sizeof(rtx_camera);
    if (bytes > c->d_views.cap) {                          // growth: queued work still reads the old array
        HIP_OK(c, hipStreamSynchronize(c->stream));
        if (int rc = ensure(c, c->d_views, bytes)) return rc;
    }
    if (int rc = stage_copy(c, c->view_ring, c->d_views.p, cameras, bytes)) return rc;
    c->view_count = view_count;
    return RTX_OK;
}

// the context's own view framebuffer: allocated on first use, grown only (the views already there are kept, new ones start at zero)
static int ensure_view_fb(rtx_ctx * c, int32_t views) {
    if (views <= c->vfb_cap) return RTX_OK;
    const size_t px = (size_t)c->cfg.width * c->cfg.height, old = (size_t)c->vfb_cap * px;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    DevBuf rgb, packed;                                             // both grown, or the old buffers stay in place
    if (int rc = grown_copy(c, c->d_vfb_rgb, old * 12, (size_t)views * px * 12, "view framebuffer", rgb)) return rc;
    if (int rc = grown_copy(c, c->d_vfb_packed, old * 4, (size_t)views * px * 4, "view framebuffer", packed)) return rc;
    c->d_vfb_rgb = std::move(rgb); c->d_vfb_packed = std::move(packed); c->vfb_cap = views;
    return RTX_OK;
}

extern "C" int rtx_render_views(rtx_ctx * c, int32_t first_view, int32_t view_count, uint32_t flags) {
    if (!c || first_view < 0 || view_count < 1 || view_count > RTX_MAX_VIEWS) return RTX_ERR_INVALID_ARG;
    if (view_pixel_count(c, view_count) >= (1ll << 31)) return RTX_ERR_INVALID_ARG;
    if (!c->frame_set) { c->err = "rtx_render_views before rtx_set_frame"; return RTX_ERR_STATE; }
    if (c->view_count == 0) { c->err = "rtx_render_views before rtx_set_views"; return RTX_ERR_STATE; }
    if ((int64_t)first_view + view_count > c->view_count) { c->err = "view range outside the views set by rtx_set_views"; return RTX_ERR_INVALID_ARG; }
    if (c->ext_vrgb) { if (first_view + view_count > c->ext_vcap) { c->err = "view range outside the bound view framebuffer"; return RTX_ERR_INVALID_ARG; } }
    else if (int rc = ensure_view_fb(c, c->view_count)) return rc;
    const int32_t tiles = frame_tiles(c);
    return render_tiles_impl(c, first_view * tiles, 1, view_count * tiles, flags, nullptr, RTX_CAM_VIEWS);
}

extern "C" int rtx_read_views(rtx_ctx * c, int32_t first_view, int32_t view_count, float * rgb_f32, uint32_t * packed_u32) {
    if (!c || first_view < 0 || view_count < 1 || view_count > RTX_MAX_VIEWS) return RTX_ERR_INVALID_ARG;
    const int32_t known_views = std::max(c->view_count, current_ray_views(c));      // the view framebuffer holds camera views and ray views alike
    if ((int64_t)first_view + view_count > known_views) { c->err = "view range outside the views set by rtx_set_views and the ray views set by rtx_set_rays / rtx_bind_rays"; return RTX_ERR_INVALID_ARG; }
    if (c->ext_vrgb && first_view + view_count > c->ext_vcap) { c->err = "view range outside the bound view framebuffer"; return RTX_ERR_INVALID_ARG; }
    hipSetDevice(c->cfg.device);
    if (!c->ext_vrgb) if (int rc = ensure_view_fb(c, known_views)) return rc;
    const size_t px = (size_t)c->cfg.width * c->cfg.height, first = (size_t)first_view * px, n = (size_t)view_count * px;
    HIP_OK(c, hipStreamSynchronize(c->stream));
    if (rgb_f32)    HIP_OK(c, hipMemcpy(rgb_f32, (const float *)(c->ext_vrgb ? c->ext_vrgb : c->d_vfb_rgb.p) + 3 * first, n * 12, hipMemcpyDeviceToHost));
    if (packed_u32) HIP_OK(c, hipMemcpy(packed_u32, (const uint32_t *)(c->ext_vpacked ? c->ext_vpacked : c->d_vfb_packed.p) + first, n * 4, hipMemcpyDeviceToHost));
    return RTX_OK;
}

// ---- ray views (include/rtx.h rtx_set_rays ...) -----------------------------------------------------------------------------------------
// A ray call is a view call whose kernels read their primary rays from a buffer of rtx_ray records instead of deriving them from a camera.
static const size_t kRayStageMax = (size_t)32 << 20;      // larger ray sets are copied synchronously instead of through the pinned ring (3 x 149 MB for one 1080p view)

extern "C" int rtx_set_rays(rtx_ctx * c, const rtx_ray * host_rays, int32_t view_count) {
    static_assert(sizeof(rtx_ray) == 72, "rtx_ray is the 18 floats of rtx_debug_trace_rays");
    if (!c || !host_rays || view_count < 1 || view_count > RTX_MAX_VIEWS) return RTX_ERR_INVALID_ARG;
    if (view_pixel_count(c, view_count) >= (1ll << 31)) { c->err = "view_count * width * height must stay below 2^31 (pixel index of a ray record)"; return RTX_ERR_INVALID_ARG; }
    hipSetDevice(c->cfg.device);
    const size_t bytes = (size_t)view_pixel_count(c, view_count) * sizeof(rtx_ray);
    if (bytes > c->d_rays.cap) {                           // growth: queued work still reads the old buffer
        HIP_OK(c, hipStreamSynchronize(c->stream));
        if (int rc = ensure(c, c->d_rays, bytes)) return rc;
    }
    if (bytes > kRayStageMax) {                            // after the work already queued (waited for), before the next call
        HIP_OK(c, hipStreamSynchronize(c->stream));
        HIP_OK(c, hipMemcpy(c->d_rays.p, host_rays, bytes, hipMemcpyHostToDevice));
        c->ray_count = view_count;
        return RTX_OK;
    }
    if (int rc = stage_copy(c, c->ray_ring, c->d_rays.p, host_rays, bytes)) return rc;
    c->ray_count = view_count;
    return RTX_OK;
}

extern "C" int rtx_bind_rays(rtx_ctx * c, const void * rays_dev, int32_t view_count) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!rays_dev) { c->ext_rays = nullptr; c->ext_ray_count = 0; return RTX_OK; }
    if (view_count < 1 || view_count > RTX_MAX_VIEWS) return RTX_ERR_INVALID_ARG;
    if (view_pixel_count(c, view_count) >= (1ll << 31)) { c->err = "view_count * width * height must stay below 2^31 (pixel index of a ray record)"; return RTX_ERR_INVALID_ARG; }
    if ((uintptr_t)rays_dev & 7u) { c->err = "the rays must be 8-byte aligned"; return RTX_ERR_INVALID_ARG; }
    // no synchronisation: work already queued keeps reading the buffer it was queued with (the pointer travels with each launch)
    c->ext_rays = rays_dev; c->ext_ray_count = view_count;
    return RTX_OK;
}

extern "C" int rtx_render_rays(rtx_ctx * c, int32_t first_view, int32_t view_count, uint32_t flags) {
    if (!c || first_view < 0 || view_count < 1 || view_count > RTX_MAX_VIEWS) return RTX_ERR_INVALID_ARG;
    if (view_pixel_count(c, view_count) >= (1ll << 31)) return RTX_ERR_INVALID_ARG;
    if (!c->frame_set) { c->err = "rtx_render_rays before rtx_set_frame"; return RTX_ERR_STATE; }
    if (c->scene.heatmap) { c->err = "rtx_render_rays in heat-map mode"; return RTX_ERR_STATE; }
    const int32_t have = current_ray_views(c);
    if (have == 0) { c->err = "rtx_render_rays before rtx_set_rays / rtx_bind_rays"; return RTX_ERR_STATE; }
    if ((int64_t)first_view + view_count > have) { c->err = "view range outside the rays set by rtx_set_rays / rtx_bind_rays"; return RTX_ERR_INVALID_ARG; }
    if (c->ext_vrgb) { if (first_view + view_count > c->ext_vcap) { c->err = "view range outside the bound view framebuffer"; return RTX_ERR_INVALID_ARG; } }
    else if (int rc = ensure_view_fb(c, std::max(have, c->view_count))) return rc;
    const int32_t tiles = frame_tiles(c);
    return render_tiles_impl(c, first_view * tiles, 1, view_count * tiles, flags, nullptr, RTX_CAM_RAYS);
}

extern "C" int rtx_bind_view_framebuffer(rtx_ctx * c, void * rgb_f32_dev, void * packed_u32_dev, int32_t view_capacity) {
    if (!c || ((rgb_f32_dev == nullptr) != (packed_u32_dev == nullptr))) return RTX_ERR_INVALID_ARG;
    if (rgb_f32_dev && view_capacity < 1) return RTX_ERR_INVALID_ARG;
    // no synchronisation: work already queued keeps writing the buffers it was queued with (the pointers travel with each launch)
    c->ext_vrgb = rgb_f32_dev; c->ext_vpacked = packed_u32_dev; c->ext_vcap = rgb_f32_dev ? view_capacity : 0;
    return RTX_OK;
}

// ---- per-pixel primary-hit AOVs (include/rtx.h rtx_bind_aovs ...) ------------------------------------------------------------------------
static const size_t kAovBytes[8] = { 4, 12, 12, 12, 8, 4, 4, 4 };        // bytes per pixel of channel k = bit 1 << k, in rtx_aov_buffers order
template <typename T> static void ** aov_slot(T & a, int k) {             // DevAov and rtx_aov_buffers: eight pointers in channel-bit order
    static_assert(sizeof(T) == 8 * sizeof(void *), "eight channel pointers");
    return reinterpret_cast<void **>(&a) + k;
}

extern "C" int rtx_bind_aovs(rtx_ctx * c, uint32_t channels, const rtx_aov_buffers * device, int64_t pixel_capacity) {
    if (!c || (channels & ~(uint32_t)RTX_AOV_ALL)) return RTX_ERR_INVALID_ARG;
    if (device && channels && pixel_capacity < 1) return RTX_ERR_INVALID_ARG;
    // no synchronisation: work already queued keeps writing the buffers it was queued with (the targets travel with each k_shade launch)
    c->aov_channels = channels;
    c->aov_ext = device != nullptr && channels != 0;
    c->aov_ext_cap = c->aov_ext ? pixel_capacity : 0;
    c->aov_ext_ptrs = DevAov{};
    if (c->aov_ext) {
        rtx_aov_buffers d = *device;
        for (int k = 0; k < 8; k++) if (channels & (1u << k)) *aov_slot(c->aov_ext_ptrs, k) = *aov_slot(d, k);
    }
    return RTX_OK;
}

// The targets of a RTX_RENDER_AOV call that writes pixels [0, pixels): the caller's buffers (capacity checked) or the context's own, grown to
// `pixels` where needed (growth waits for queued work, which may still write the old buffers; the pixels already there are kept).
static int aov_targets_of_call(rtx_ctx * c, int64_t pixels, DevAov & out) {
    out = DevAov{};
    if (c->aov_ext) {
        if (pixels > c->aov_ext_cap) { c->err = "the call's pixel range exceeds the pixel_capacity of the bound AOV buffers"; return RTX_ERR_INVALID_ARG; }
        out = c->aov_ext_ptrs;
        return RTX_OK;
    }
    for (int k = 0; k < 8; k++) {
        if (!(c->aov_channels & (1u << k))) continue;
        if (pixels > c->aov_own_cap[k]) {
            HIP_OK(c, hipStreamSynchronize(c->stream));
            if (int rc = grow_keep(c, c->d_aov[k], (size_t)c->aov_own_cap[k] * kAovBytes[k], (size_t)pixels * kAovBytes[k], "AOV buffer")) return rc;
            c->aov_own_cap[k] = pixels;
        }
        *aov_slot(out, k) = c->d_aov[k].p;
    }
    return RTX_OK;
}

extern "C" int rtx_read_aovs(rtx_ctx * c, int32_t first_view, int32_t view_count, const rtx_aov_buffers * host) {
    if (!c || !host || first_view < 0 || view_count < 1) return RTX_ERR_INVALID_ARG;
    if (c->aov_ext) { c->err = "rtx_read_aovs while caller AOV buffers are bound"; return RTX_ERR_STATE; }
    const int64_t px = (int64_t)c->cfg.width * c->cfg.height, first = first_view * px, n = view_count * px;
    rtx_aov_buffers h = *host;
    for (int k = 0; k < 8; k++)
        if (*aov_slot(h, k) && first + n > c->aov_own_cap[k]) { c->err = "rtx_read_aovs: a requested channel's own buffer does not hold the range"; return RTX_ERR_INVALID_ARG; }
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 8; k++)
        if (void * dst = *aov_slot(h, k)) HIP_OK(c, hipMemcpy(dst, (const char *)c->d_aov[k].p + (size_t)first * kAovBytes[k], (size_t)n * kAovBytes[k], hipMemcpyDeviceToHost));
    return RTX_OK;
}

extern "C" int rtx_enable_kernel_timing(rtx_ctx * c, int32_t enable) {
    if (!c) return RTX_ERR_INVALID_ARG;
    c->timing = enable != 0;
    c->times.clear(); c->event_next = 0;      // launches are recorded from now on, across render calls
    return RTX_OK;
}

extern "C" int rtx_last_kernel_times(rtx_ctx * c, const char ** names, float * ms, int32_t capacity, int32_t * count) {
    if (!c || !count) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    *count = (int32_t)c->times.size();
    for (int i = 0; i < (int)c->times.size() && i < capacity; i++) {
        float t = 0.0f;
        hipEventElapsedTime(&t, c->times[i].a, c->times[i].b);
        if (names) names[i] = c->times[i].name;
        if (ms) ms[i] = t;
    }
    return RTX_OK;
}

// ---- unit-level entry points (parity tests of single reference functions on the device) --------------
__global__ void k_debug_libm(int fn, const float * a, const float * b, float * out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r;
    switch (fn) {
        case 0: r = rtx_acosf(a[i]); break;
        case 1: r = rtx_atan2f(a[i], b[i]); break;
        case 2: r = rtx_expf(a[i]); break;
        case 3: r = rtx_log2f(a[i]); break;
        case 4: r = rtx_atanf(a[i]); break;
        case 5: r = (float)f2i_rn_x86(a[i]); break;
        case 6: r = 1.0f / sqrtf(a[i]); break;                  // the reciprocal length of vnormalize
        case 7: r = (float)f2i_trunc_x86(a[i]); break;
        case 8: r = pow2_128(a[i]); break;
        default: return;                                        // rtx_debug_libm refuses every other id before the launch
    }
    out[i] = r;
}

extern "C" int rtx_debug_libm(rtx_ctx * c, int32_t fn, const float * a, const float * b, float * out, int32_t n) {
    if (!c || !a || !out || n <= 0 || fn < 0 || fn > 8) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    DevBuf da, db, dout;                 // scratch of this call: released on every way out
    int rc = upload(c, da, a, (size_t)n * 4);
    if (!rc) rc = upload(c, db, b ? b : a, (size_t)n * 4);
    if (!rc) rc = ensure(c, dout, (size_t)n * 4);
    if (rc) return rc;
    hipLaunchKernelGGL(k_debug_libm, dim3((n + 255) / 256), dim3(256), 0, c->stream, fn, (const float *)da.p, (const float *)db.p, (float *)dout.p, n);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    HIP_OK(c, hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RTX_OK;
}

__global__ void k_debug_texture(DevScene sc, int tex, const float * in6, float * out3, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    TexCtx tc; tc.t = &sc.textures[tex]; tc.fetches = 0;
    const float * p = in6 + 6 * (size_t)i;
    const v3 r = texture_sample(tc, sc, p[0], p[1], p[2], p[3], p[4], p[5]);
    out3[3 * i] = r.x; out3[3 * i + 1] = r.y; out3[3 * i + 2] = r.z;
}

// Texture::sample (Texture.h:33-49) at n (s, t, ds_dx, ds_dy, dt_dx, dt_dy) inputs with the context's texture_mode / mip_filter
extern "C" int rtx_debug_texture_sample(rtx_ctx * c, int32_t texture_id, const float * in6, float * out3, int32_t n) {
    if (!c || !in6 || !out3 || n <= 0 || texture_id < 0 || (size_t)texture_id >= c->h_tex.size() || !c->h_tex[texture_id].texels) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    DevScene sc = c->scene;
    sc.texture_mode = c->cfg.texture_mode; sc.mip_filter = c->cfg.mip_filter; sc.max_anisotropy = c->cfg.max_anisotropy;
    sc.ewa_table = (const float *)c->d_ewa.p;                  // the texture table is bound since rtx_create (bind_tables)
    DevBuf din, dout;
    int rc = upload(c, din, in6, (size_t)n * 24);
    if (!rc) rc = ensure(c, dout, (size_t)n * 12);
    if (rc) return rc;
    hipLaunchKernelGGL(k_debug_texture, dim3((n + 255) / 256), dim3(256), 0, c->stream, sc, texture_id, (const float *)din.p, (float *)dout.p, n);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    HIP_OK(c, hipMemcpy(out3, dout.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    return RTX_OK;
}

__global__ void k_debug_sky(const float * sky, int size, const float * dirs, float * out3, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const v3 r = sky_sample(sky, size, V3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
    out3[3 * i] = r.x; out3[3 * i + 1] = r.y; out3[3 * i + 2] = r.z;
}

// which shadow-ray walk an uploaded mesh gets: the stack need of its 4-wide records, or -1 for the binary walk
extern "C" int rtx_debug_blas_wide(rtx_ctx * c, int32_t blas_id, int32_t * stack_need) {
    if (!c || !stack_need || blas_id < 0 || (size_t)blas_id >= c->h_blas.size() || !c->h_blas[blas_id].nodes) return RTX_ERR_INVALID_ARG;
    *stack_need = c->h_blas[blas_id].pk4_nodes ? c->h_blas[blas_id].pk4_need : -1;
    return RTX_OK;
}

// which per-lane closest-hit walk an uploaded mesh gets: the stack need of its ordered 4-wide records, or -1 for the binary walk
extern "C" int rtx_debug_blas_wide_closest(rtx_ctx * c, int32_t blas_id, int32_t * stack_need) {
    if (!c || !stack_need || blas_id < 0 || (size_t)blas_id >= c->h_blas.size() || !c->h_blas[blas_id].nodes) return RTX_ERR_INVALID_ARG;
    *stack_need = c->h_blas[blas_id].pk4c_nodes ? c->h_blas[blas_id].pk4c_need : -1;
    return RTX_OK;
}

// the grids rtx_create sized (from the device, RTX_GRID_CUS and the grid knobs), as the launches use them: launches nothing, waits for nothing
extern "C" int rtx_debug_grids(rtx_ctx * c, int32_t out[8]) {
    if (!c || !out) return RTX_ERR_INVALID_ARG;
    out[0] = c->n_cu; out[1] = c->trace_blocks_closest; out[2] = c->trace_blocks_any; out[3] = c->trace_blocks_count;
    out[4] = c->pk_blocks_closest; out[5] = c->pk_blocks_any; out[6] = c->item_blocks; out[7] = c->q.spill_threads;
    return RTX_OK;
}

// Sky::sample (Sky.cpp:28-68) at n directions
extern "C" int rtx_debug_sky_sample(rtx_ctx * c, const float * dirs3, float * out3, int32_t n) {
    if (!c || !dirs3 || !out3 || n <= 0) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    DevBuf din, dout;
    int rc = upload(c, din, dirs3, (size_t)n * 12);
    if (!rc) rc = ensure(c, dout, (size_t)n * 12);
    if (rc) return rc;
    hipLaunchKernelGGL(k_debug_sky, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const float *)c->d_sky.p, c->sky_size, (const float *)din.p, (float *)dout.p, n);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    HIP_OK(c, hipMemcpy(out3, dout.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    return RTX_OK;
}


// ---- GPU groups: screen tiles sharded over the GPUs of one node, RCCL gather of the packed tiles to rank 0 -----------
// RCCL is bound at run time (dlopen): librtx_hip.so has no link-time dependency on it, and a process that already carries an RCCL
// (e.g. PyTorch's) gets that same copy.
#include <dlfcn.h>
typedef struct { char internal[128]; } rtx_nccl_id;
typedef void * rtx_nccl_comm;
struct RcclApi {
    void * lib = nullptr;
    int (*GetUniqueId)(rtx_nccl_id *) = nullptr;
    int (*CommInitRank)(rtx_nccl_comm *, int, rtx_nccl_id, int) = nullptr;
    int (*CommInitAll)(rtx_nccl_comm *, int, const int *) = nullptr;
    int (*CommDestroy)(rtx_nccl_comm) = nullptr;
    int (*Gather)(const void *, void *, size_t, int, int, rtx_nccl_comm, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char * (*GetErrorString)(int) = nullptr;
};
static RcclApi * rccl() {
    static RcclApi api; static bool tried = false;
    if (tried) return api.lib ? &api : nullptr;
    tried = true;
    const char * names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
    for (const char * n : names) { api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL); if (api.lib) break; }
    if (!api.lib) return nullptr;
    bool ok = true;
    auto sym = [&](const char * n) { void * p = dlsym(api.lib, n); if (!p) ok = false; return p; };
    api.GetUniqueId = (int (*)(rtx_nccl_id *))sym("ncclGetUniqueId");
    api.CommInitRank = (int (*)(rtx_nccl_comm *, int, rtx_nccl_id, int))sym("ncclCommInitRank");
    api.CommInitAll = (int (*)(rtx_nccl_comm *, int, const int *))sym("ncclCommInitAll");
    api.CommDestroy = (int (*)(rtx_nccl_comm))sym("ncclCommDestroy");
    api.Gather = (int (*)(const void *, void *, size_t, int, int, rtx_nccl_comm, hipStream_t))sym("ncclGather");
    api.GroupStart = (int (*)())sym("ncclGroupStart");
    api.GroupEnd = (int (*)())sym("ncclGroupEnd");
    api.GetErrorString = (const char * (*)(int))sym("ncclGetErrorString");
    if (!ok) { dlclose(api.lib); api.lib = nullptr; return nullptr; }
    return &api;
}

// One communicator per rank, shared by every context of that rank that joins it (rtx_group_attach: further frames in flight on the same GPU).
// With more than one member the gathers are issued on the hub's own exchange stream, in call order: every rank issues them in the same
// order whatever order its frames finish rendering in, and no two collectives of a rank are ever in flight at once.
struct GroupHub { rtx_nccl_comm comm = nullptr; hipStream_t xs = nullptr; int refs = 1; int device = 0; };
struct rtx_group {
    rtx_ctx * ctx = nullptr;
    int rank = 0, world = 1, tiles_total = 0, tiles_per_rank = 0, own_tiles = 0;
    GroupHub * hub = nullptr;
    hipEvent_t ev_rendered = nullptr, ev_gathered = nullptr;
    DevBuf send, recv;           // tile-major packed pixels: this rank's tiles; on rank 0 every rank's
};

static int group_setup(rtx_group * g) {
    rtx_ctx * c = g->ctx;
    g->tiles_total = frame_tiles(c);
    g->tiles_per_rank = group_tiles_per_rank(g->tiles_total, g->world);      // padded: every rank sends the same count
    g->own_tiles = group_own_tiles(g->tiles_total, g->world, g->rank);
    hipSetDevice(c->cfg.device);
    int rc = ensure(c, g->send, (size_t)g->tiles_per_rank * 1024 * 4);
    if (!rc && g->rank == 0) rc = ensure(c, g->recv, (size_t)g->world * g->tiles_per_rank * 1024 * 4);
    // the padding tiles are never written by a render: zero them once, ordered before the first render on the context's own stream
    if (!rc) HIP_OK(c, hipMemsetAsync(g->send.p, 0, (size_t)g->tiles_per_rank * 1024 * 4, c->stream));
    return rc;
}

// The partition and the tile-major slot order as plain host functions (no GPU needed): what rank `rank` of `world` renders and where
// each of its pixels travels in the gather.  They call the very functions the kernels use (rtx_trace.h: group_*, tile_slot_pixel).
extern "C" int rtx_group_layout(int32_t width, int32_t height, int32_t world, int32_t rank, int32_t * tiles_total, int32_t * tiles_per_rank, int32_t * own_tiles) {
    if (width <= 0 || height <= 0 || world < 1 || rank < 0 || rank >= world) return RTX_ERR_INVALID_ARG;
    const int tcx = (width + RTX_TILE_SIZE - 1) / RTX_TILE_SIZE, tcy = (height + RTX_TILE_SIZE - 1) / RTX_TILE_SIZE;
    if (tiles_total) *tiles_total = tcx * tcy;
    if (tiles_per_rank) *tiles_per_rank = group_tiles_per_rank(tcx * tcy, world);
    if (own_tiles) *own_tiles = group_own_tiles(tcx * tcy, world, rank);
    return RTX_OK;
}

// pixel_index[i] = raster index (y * width + x) of slot i of the rank's send buffer (tiles_per_rank * 1024 slots), or -1 for padding
// (clipped pixels of edge tiles, the unused tail when the tiles do not divide evenly).  Rank 0's receive buffer is the concatenation
// of every rank's send buffer in rank order, which is all k_unswizzle relies on.
extern "C" int rtx_group_slot_pixels(int32_t width, int32_t height, int32_t world, int32_t rank, int64_t * pixel_index, int64_t capacity) {
    int32_t total = 0, per_rank = 0, own = 0;
    const int rc = rtx_group_layout(width, height, world, rank, &total, &per_rank, &own);
    if (rc) return rc;
    if (!pixel_index || capacity < (int64_t)per_rank * 1024) return RTX_ERR_INVALID_ARG;
    const int tcx = (width + RTX_TILE_SIZE - 1) / RTX_TILE_SIZE;
    for (int k = 0; k < per_rank; k++) {
        const int tile = group_tile_of(world, rank, k);
        for (int l = 0; l < 1024; l++) {
            int px, py; tile_slot_pixel(tile, l, tcx, px, py);
            pixel_index[(int64_t)k * 1024 + l] = (k < own && tile < total && px < width && py < height) ? (int64_t)py * width + px : -1;
        }
    }
    return RTX_OK;
}

extern "C" int rtx_group_unique_id(void * id128) {
    if (!id128) return RTX_ERR_INVALID_ARG;
    RcclApi * r = rccl();
    if (!r) return RTX_ERR_STATE;
    rtx_nccl_id id;
    if (r->GetUniqueId(&id) != 0) return RTX_ERR_HIP;
    memcpy(id128, &id, sizeof(id));
    return RTX_OK;
}

extern "C" int rtx_group_create(rtx_ctx * c, int32_t rank, int32_t world, const void * id128, rtx_group ** out) {
    if (!c || !out || world < 1 || rank < 0 || rank >= world || (world > 1 && !id128)) return RTX_ERR_INVALID_ARG;
    *out = nullptr;
    rtx_group * g = new rtx_group();
    g->ctx = c; g->rank = rank; g->world = world;
    RcclApi * r = rccl();
    if (!r) { c->err = "RCCL (librccl.so.1) could not be loaded"; delete g; return RTX_ERR_STATE; }
    hipSetDevice(c->cfg.device);
    rtx_nccl_id id; memset(&id, 0, sizeof(id));
    if (id128) memcpy(&id, id128, sizeof(id)); else if (r->GetUniqueId(&id) != 0) { delete g; return RTX_ERR_HIP; }
    g->hub = new GroupHub(); g->hub->device = c->cfg.device;
    const int e = r->CommInitRank(&g->hub->comm, world, id, rank);
    if (e != 0) { c->err = std::string("ncclCommInitRank: ") + r->GetErrorString(e); delete g->hub; delete g; return RTX_ERR_HIP; }
    const int rc = group_setup(g);
    if (rc) { r->CommDestroy(g->hub->comm); delete g->hub; delete g; return rc; }
    *out = g;
    return RTX_OK;
}

// A further context of the same process and GPU (another frame in flight) joins `base`'s communicator as the same rank.
extern "C" int rtx_group_attach(rtx_ctx * c, rtx_group * base, rtx_group ** out) {
    if (!c || !base || !base->hub || !out || c == base->ctx || c->cfg.device != base->hub->device ||
        c->cfg.width != base->ctx->cfg.width || c->cfg.height != base->ctx->cfg.height) return RTX_ERR_INVALID_ARG;
    *out = nullptr;
    hipSetDevice(c->cfg.device);
    GroupHub * h = base->hub;
    if (!h->xs) {      // the exchange stream gets the highest priority: RCCL's copy kernel needs a few workgroups' worth of room beside the frames' persistent grids, and should be first in line for it
        int lo = 0, hi = 0;
        hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (knob_int("RTX_XS_PRIORITY", 1, 0, 1)) HIP_OK(c, hipStreamCreateWithPriority(&h->xs, hipStreamNonBlocking, hi));
        else HIP_OK(c, hipStreamCreateWithFlags(&h->xs, hipStreamNonBlocking));
    }
    rtx_group * g = new rtx_group();
    g->ctx = c; g->rank = base->rank; g->world = base->world; g->hub = h; h->refs++;
    const int rc = group_setup(g);
    if (rc) { h->refs--; delete g; return rc; }
    *out = g;
    return RTX_OK;
}

// One process driving n GPUs (the shape of the reference's own main loop): contexts[i] lives on its own device and becomes rank i.
extern "C" int rtx_group_create_local(rtx_ctx ** contexts, int32_t n, rtx_group ** out_groups) {
    if (!contexts || !out_groups || n < 1 || n > 64) return RTX_ERR_INVALID_ARG;
    RcclApi * r = rccl();
    if (!r) return RTX_ERR_STATE;
    std::vector<int> devs(n); std::vector<rtx_nccl_comm> comms(n, nullptr);
    for (int i = 0; i < n; i++) { if (!contexts[i]) return RTX_ERR_INVALID_ARG; devs[i] = contexts[i]->cfg.device; out_groups[i] = nullptr; }
    const int e = r->CommInitAll(comms.data(), n, devs.data());
    if (e != 0) { contexts[0]->err = std::string("ncclCommInitAll: ") + r->GetErrorString(e); return RTX_ERR_HIP; }
    int rc = RTX_OK;
    for (int i = 0; i < n; i++) {                                   // every communicator gets an owner first, so that one rollback path frees them all
        rtx_group * g = new rtx_group();
        g->ctx = contexts[i]; g->rank = i; g->world = n; g->hub = new GroupHub(); g->hub->comm = comms[i]; g->hub->device = devs[i];
        out_groups[i] = g;
    }
    for (int i = 0; i < n && !rc; i++) rc = group_setup(out_groups[i]);
    if (rc) { for (int i = 0; i < n; i++) { rtx_group_destroy(out_groups[i]); out_groups[i] = nullptr; } }
    return rc;
}

static int group_render_one(rtx_group * g, uint32_t flags, bool render, bool gather, bool finish) {
    rtx_ctx * c = g->ctx;
    RcclApi * r = rccl();
    hipSetDevice(c->cfg.device);
    if (render) {
        const int rc = render_tiles_impl(c, g->rank, g->world, g->own_tiles, flags | RTX_RENDER_SERIAL, (uint32_t *)g->send.p);
        if (rc) return rc;
    }
    if (gather) {
        // the one exchange of a frame: every rank's tiles_per_rank * 4 KiB of packed pixels to rank 0, on the stream the frame was rendered on
        hipStream_t xs = c->stream;
        if (g->hub->xs) {                                   // shared communicator: the exchange stream orders this rank's collectives
            if (!g->ev_rendered) { HIP_OK(c, hipEventCreateWithFlags(&g->ev_rendered, hipEventDisableTiming)); HIP_OK(c, hipEventCreateWithFlags(&g->ev_gathered, hipEventDisableTiming)); }
            xs = g->hub->xs;
            HIP_OK(c, hipEventRecord(g->ev_rendered, c->stream)); HIP_OK(c, hipStreamWaitEvent(xs, g->ev_rendered, 0));
        }
        const int e = r->Gather(g->send.p, g->recv.p, (size_t)g->tiles_per_rank * 1024, /*ncclUint32*/ 3, 0, g->hub->comm, xs);
        if (e != 0) { c->err = std::string("ncclGather: ") + r->GetErrorString(e); return RTX_ERR_HIP; }
        if (xs != c->stream) { HIP_OK(c, hipEventRecord(g->ev_gathered, xs)); HIP_OK(c, hipStreamWaitEvent(c->stream, g->ev_gathered, 0)); }
    }
    if (finish && g->rank == 0) {
        const int tcx = (c->cfg.width + RTX_TILE_SIZE - 1) / RTX_TILE_SIZE;
        hipLaunchKernelGGL(k_unswizzle, dim3(c->n_cu * 4), dim3(256), 0, c->stream, (const uint32_t *)g->recv.p,
                           (uint32_t *)(c->ext_packed ? c->ext_packed : c->d_fb_packed.p), g->world, g->tiles_per_rank, g->tiles_total, tcx, c->cfg.width, c->cfg.height);
        HIP_OK(c, hipGetLastError());
    }
    return RTX_OK;
}

// Renders this rank's tile shard (tile t belongs to rank t mod world, WorkerThread.cpp:53-65 without the atomic counter), gathers the
// packed tiles to rank 0 and, there, writes the frame into the context's packed framebuffer.  Everything is queued on the context's
// stream; nothing synchronises with the host.
extern "C" int rtx_group_render(rtx_group * g, uint32_t flags) {
    if (!g || !g->ctx || (flags & RTX_RENDER_AOV)) return RTX_ERR_INVALID_ARG;      // AOVs are not supported on the group path
    return group_render_one(g, flags, true, true, true);
}

extern "C" int rtx_group_render_local(rtx_group ** groups, int32_t n, uint32_t flags) {
    if (!groups || n < 1 || (flags & RTX_RENDER_AOV)) return RTX_ERR_INVALID_ARG;
    RcclApi * r = rccl();
    if (!r) return RTX_ERR_STATE;
    for (int i = 0; i < n; i++) { if (!groups[i]) return RTX_ERR_INVALID_ARG; const int rc = group_render_one(groups[i], flags, true, false, false); if (rc) return rc; }
    r->GroupStart();                                               // one thread issues every rank's call of the collective
    int rc = RTX_OK;
    for (int i = 0; i < n && !rc; i++) rc = group_render_one(groups[i], flags, false, true, false);
    r->GroupEnd();
    for (int i = 0; i < n && !rc; i++) rc = group_render_one(groups[i], flags, false, false, true);
    return rc;
}

extern "C" int rtx_group_destroy(rtx_group * g) {
    if (!g) return RTX_ERR_INVALID_ARG;
    if (g->ctx) { hipSetDevice(g->ctx->cfg.device); if (g->ctx->stream) hipStreamSynchronize(g->ctx->stream); }
    if (g->hub) {
        if (g->hub->xs) hipStreamSynchronize(g->hub->xs);
        if (--g->hub->refs == 0) { RcclApi * r = rccl(); if (r && g->hub->comm) r->CommDestroy(g->hub->comm); if (g->hub->xs) hipStreamDestroy(g->hub->xs); delete g->hub; }
    }
    if (g->ev_rendered) hipEventDestroy(g->ev_rendered);
    if (g->ev_gathered) hipEventDestroy(g->ev_gathered);
    delete g;                            // with its send / recv buffers
    return RTX_OK;
}

// Test hook: the whole group path of `world` ranks on ONE GPU without RCCL — every rank's tile shard rendered tile-major straight into
// its slice of rank 0's receive buffer, then the same k_unswizzle.  Covers the partition, the tile-major writes and the frame assembly
// for any world size; the ncclGather itself is exercised by rtx_group_render.
extern "C" int rtx_debug_group_loopback(rtx_ctx * c, int32_t world, uint32_t flags) {
    if (!c || world < 1 || (flags & RTX_RENDER_AOV)) return RTX_ERR_INVALID_ARG;
    rtx_group g; g.ctx = c; g.rank = 0; g.world = world;
    int rc = group_setup(&g);
    for (int r = 0; r < world && !rc; r++) {
        const int own = group_own_tiles(g.tiles_total, world, r);
        rc = render_tiles_impl(c, r, world, own, flags | RTX_RENDER_SERIAL, (uint32_t *)g.recv.p + (size_t)r * g.tiles_per_rank * 1024);
    }
    if (!rc) {
        const int tcx = (c->cfg.width + RTX_TILE_SIZE - 1) / RTX_TILE_SIZE;
        hipLaunchKernelGGL(k_unswizzle, dim3(c->n_cu * 4), dim3(256), 0, c->stream, (const uint32_t *)g.recv.p,
                           (uint32_t *)(c->ext_packed ? c->ext_packed : c->d_fb_packed.p), world, g.tiles_per_rank, g.tiles_total, tcx, c->cfg.width, c->cfg.height);
    }
    hipStreamSynchronize(c->stream);     // before g's buffers go: what was queued writes them
    return rc;
}

// ---- ray queries (include/rtx.h: rtx_query_closest / rtx_query_occluded; kernels in rtx_query.h) -------------------------------------
// N rays or segments in device memory against the frame the context holds, answers into device memory: per chunk of at most
// RTX_QUERY_CHUNK_RAYS rows  k_begin_batch -> fill -> the production traversal kernel -> resolve / store, all on the context's stream; with
// RTX_QUERY_SORT the round starts with bounds -> keys -> rocPRIM's radix sort, and the fill and the resolve / store go through the sorted keys.
// Nothing here waits, copies or allocates once the scratch holds a chunk of the call's size.
//
// The queue set is the queries' own; the frame's (alloc_queues, c->q, d_counters) belongs to render calls.  Level 1 for rays and hits,
// level 0 for the node flags of the one explicit shadow segment, both at base 0 — a closest-hit query touches r0 / r1 / h0 / h1, an
// occlusion query s0 / s1 / n0 / socc, and the two are stream-ordered, so they share four buffers: 52 bytes per slot, 52 MiB for a full
// chunk.  DevScene and DevQueues travel by value: a frame queued before or after is untouched.  The unit-test hooks rtx_debug_trace_rays /
// rtx_debug_occluded (further down) run the same setup and the same rounds from host arrays.
//
// RTX_QUERY_SORT (sort != null) adds a block of its own, made by the first sorted call and grown only: [unsorted keys][sorted keys][bounds]
// [rocPRIM's temporary storage], 2 x 8 bytes per slot and what rocPRIM asks for a round of that many keys (a host-side query).  Both blocks
// grow in the one branch that waits; a context that never sorts never allocates the second.
struct QuerySort { uint64_t * keys_in, * keys; uint32_t * bounds; void * tmp; size_t tmp_bytes; };
static int query_queues(rtx_ctx * c, int64_t n, DevQueues * qp, QuerySort * sort = nullptr) {      // qp == null: only the sort block (the walk queries have no queue set)
    const int64_t rows = n < (int64_t)RTX_QUERY_CHUNK_RAYS ? n : (int64_t)RTX_QUERY_CHUNK_RAYS;
    const int32_t cap = (int32_t)((rows + RTX_WAVE - 1) & ~(int64_t)(RTX_WAVE - 1));      // whole packets: the fill marks the tail of the last one
    size_t sort_tmp = 0;
    if (sort) {                                            // the largest round and the last one: rocPRIM picks its method by the count
        size_t last = 0;
        if (int rc = sort_storage_bytes<uint64_t>(c, (size_t)rows, (unsigned int)rtxq::KEY_BITS, sort_tmp)) return rc;
        if (int rc = sort_storage_bytes<uint64_t>(c, (size_t)(n - (n - 1) / RTX_QUERY_CHUNK_RAYS * RTX_QUERY_CHUNK_RAYS), (unsigned int)rtxq::KEY_BITS, last)) return rc;
        if (last > sort_tmp) sort_tmp = last;
    }
    const bool grow_sort = sort && (cap > c->query_sort_cap || sort_tmp > c->query_sort_tmp);
    const bool grow_rays = qp && cap > c->query_cap;
    if (grow_rays || grow_sort) {                          // growth: queued queries still use the old buffers
        HIP_OK(c, hipStreamSynchronize(c->stream));
        if (grow_rays) {
            int rc = ensure(c, c->d_query_counters, sizeof(DevCounters));
            if (!rc) rc = ensure(c, c->d_query_heads, (size_t)2 * (RTX_MAX_LEVELS + 1) * RTX_PK_CLASSES * 32 * sizeof(uint32_t));
            for (int k = 0; k < 4 && !rc; k++) rc = ensure(c, c->d_query[k], (size_t)cap * (k < 3 ? 16 : 4));
            if (rc) { c->query_cap = 0; return rc; }
            c->query_cap = cap;
        }
        if (grow_sort) {
            const int32_t scap = cap > c->query_sort_cap ? cap : c->query_sort_cap;
            const size_t stmp = sort_tmp > c->query_sort_tmp ? sort_tmp : c->query_sort_tmp;
            const size_t len[4] = { (size_t)scap * 8, (size_t)scap * 8, 2 * rtxq::COORDS * sizeof(uint32_t), stmp };
            size_t off[4];
            if (int rc = ensure(c, c->d_query_sort, aligned_parts(len, off, 4))) { c->query_sort_cap = 0; c->query_sort_tmp = 0; return rc; }
            c->query_sort_cap = scap; c->query_sort_tmp = stmp;
        }
    }
    if (sort) {
        const size_t len[4] = { (size_t)c->query_sort_cap * 8, (size_t)c->query_sort_cap * 8, 2 * rtxq::COORDS * sizeof(uint32_t), c->query_sort_tmp };
        size_t off[4];
        aligned_parts(len, off, 4);
        char * const sb = (char *)c->d_query_sort.p;
        sort->keys_in = (uint64_t *)(sb + off[0]); sort->keys = (uint64_t *)(sb + off[1]); sort->bounds = (uint32_t *)(sb + off[2]);
        sort->tmp = sb + off[3]; sort->tmp_bytes = c->query_sort_tmp;
    }
    if (!qp) return RTX_OK;
    DevQueues & q = *qp;
    q = c->q;                                              // the walkers' knobs (thresholds, spill_threads) as rtx_create read them
    for (int d = 0; d <= RTX_MAX_LEVELS; d++) { q.level_base[d] = 0; q.level_cap[d] = d < 2 ? c->query_cap : 0; q.shadow_base[d] = 0; q.stats_n[d] = 0; }
    q.first_tile = 0; q.tile_stride = 1; q.tile_count = 0; q.primary_slots = 0;
    q.r0 = q.s0 = (float4 *)c->d_query[0].p; q.r1 = q.s1 = (float4 *)c->d_query[1].p; q.h0 = q.n0 = (float4 *)c->d_query[2].p;
    q.h1 = (int32_t *)c->d_query[3].p; q.socc = (uint32_t *)c->d_query[3].p;
    q.r2 = q.r3 = q.r4 = q.n1 = q.n2 = q.c0 = q.c1 = q.sp = q.sn = nullptr; q.views = nullptr;
    q.shadow_explicit = 0; q.cull = 0;
    q.spill = (int32_t *)c->d_spill.p; q.pk_fifo = (int32_t *)c->d_pk_fifo.p;
    q.pk_items = nullptr; q.pk_item_count = nullptr; q.pk_item_cap = 0;
    q.counters = (DevCounters *)c->d_query_counters.p; q.pk_heads = (uint32_t *)c->d_query_heads.p;
    q.stats_partial = nullptr; q.stats_stride = 0; q.pk_cost = nullptr; q.pk_lpt_order = nullptr;
    q.tm_packed = nullptr; q.tm_base = 0; q.fb_rgb = nullptr; q.fb_packed = nullptr;
    return RTX_OK;
}

// RTX_QUERY_SORT, one round: the bounds of the m rows at `rows` (ROW floats each), their keys, rocPRIM's radix sort -> S.keys, the order
// the fill gathers by and the resolve scatters by.  Three launches and a 48-byte memset on the stream; the host learns nothing.
// KEY < ROW: the key is taken over the first KEY floats of every row (rtx_query_sweep: the 7-float key of its 8-float rows).
template <int ROW, int KEY = ROW> static int query_sort_round(rtx_ctx * c, const QuerySort & S, const float * rows, int m) {
    const dim3 grid((m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK), block(RTX_QUERY_BLOCK);
    HIP_OK(c, hipMemsetAsync(S.bounds, 0xff, 2 * rtxq::COORDS * sizeof(uint32_t), c->stream));
    if constexpr (KEY == ROW) {
        launch_timed(c, "k_query_sort_bounds", c->stream, [&] { hipLaunchKernelGGL((k_query_sort_bounds<ROW>), grid, block, 0, c->stream, rows, m, S.bounds); });
        launch_timed(c, "k_query_sort_keys", c->stream, [&] { hipLaunchKernelGGL((k_query_sort_keys<ROW>), grid, block, 0, c->stream, rows, m, (const uint32_t *)S.bounds, S.keys_in); });
    } else {
        launch_timed(c, "k_query_sort_bounds", c->stream, [&] { hipLaunchKernelGGL((k_query_sort_bounds_of<ROW, KEY>), grid, block, 0, c->stream, rows, m, S.bounds); });
        launch_timed(c, "k_query_sort_keys", c->stream, [&] { hipLaunchKernelGGL((k_query_sort_keys_of<ROW, KEY>), grid, block, 0, c->stream, rows, m, (const uint32_t *)S.bounds, S.keys_in); });
    }
    hipError_t se = hipSuccess;
    launch_timed(c, "query_radix_sort", c->stream, [&] { size_t bytes = S.tmp_bytes; se = rocprim::radix_sort_keys(S.tmp, bytes, (const uint64_t *)S.keys_in, S.keys, (unsigned int)m, 0u, (unsigned int)rtxq::KEY_BITS, c->stream); });
    if (se != hipSuccess) return sort_failed(c, se);
    return RTX_OK;
}

// the checks the two queries and the two debug hooks share, in the order the header lists them; nothing is queued on an error
static int query_checks(rtx_ctx * c, const void * in, int64_t n, const void * out, uint32_t flags, const char * what,
                        uint32_t allowed = RTX_RENDER_LANE_TRACE | RTX_RENDER_PACKET_CLOSEST | RTX_QUERY_SORT) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!in || !out || n < 1) { c->err = std::string(what) + ": null pointer or n < 1"; return RTX_ERR_INVALID_ARG; }
    if (flags & ~allowed) {
        c->err = std::string(what) + (allowed == (uint32_t)RTX_QUERY_SORT ? ": flags other than RTX_QUERY_SORT" :
                                      (allowed & (uint32_t)RTX_OVERLAP_ANY) ? ": flags other than RTX_QUERY_SORT / RTX_OVERLAP_OBJECTS / RTX_OVERLAP_ANY" :
                                      ": flags other than RTX_RENDER_LANE_TRACE / RTX_RENDER_PACKET_CLOSEST / RTX_QUERY_SORT");
        return RTX_ERR_INVALID_ARG;
    }
    if (!c->frame_set) { c->err = std::string(what) + " before rtx_set_frame"; return RTX_ERR_STATE; }
    if (c->scene.heatmap) { c->err = std::string(what) + " in heat-map mode"; return RTX_ERR_STATE; }
    return validate_references(c);
}

// What a call decides once for all its rounds: the queue set, the sorted keys of a round (order; null = the caller's order), the kernels the
// stack rule leaves the flags, the scene by value.  The two queries and the two debug hooks all start here.
struct QueryCall { DevQueues q; QuerySort S; const uint64_t * order; bool lane; DevScene sc; };
static int query_setup(rtx_ctx * c, const void * in, int64_t n, const void * out, uint32_t flags, const char * what, QueryCall & k) {
    if (int bad = query_checks(c, in, n, out, flags, what)) return bad;
    hipSetDevice(c->cfg.device);
    const bool sorted = (flags & RTX_QUERY_SORT) != 0;
    if (int rc = query_queues(c, n, &k.q, sorted ? &k.S : nullptr)) return rc;
    k.order = sorted ? k.S.keys : nullptr;
    k.lane = (flags & RTX_RENDER_LANE_TRACE) != 0;
    bool pk_closest = (flags & RTX_RENDER_PACKET_CLOSEST) != 0;
    plan_stack_limits(stack_figures(c), k.lane, pk_closest);
    if (pk_closest) k.q.pk_defer_t0_closest = k.q.pk_defer_t0_primary = k.q.pk_defer_t0;      // thresholds only closest-hit packets read
    k.sc = c->scene;
    return RTX_OK;
}

// The rounds of a call over n rows: round(first, m) queues rows [first, first + m), m <= RTX_QUERY_CHUNK_RAYS, back to back.  q: the call's
// queue set, null for the walk queries, which have none
template <typename F> static int query_rounds(rtx_ctx * c, DevQueues * q, int64_t n, F && round) {
    for (int64_t first = 0; first < n; first += RTX_QUERY_CHUNK_RAYS) {
        const int m = (int)(n - first < (int64_t)RTX_QUERY_CHUNK_RAYS ? n - first : (int64_t)RTX_QUERY_CHUNK_RAYS);
        if (q) q->tile_count = (m + 1023) / 1024;
        if (int rc = round(first, m)) return rc;
    }
    HIP_OK(c, hipGetLastError());
    return RTX_OK;
}
// The channel targets of the round that starts at caller row `first`: the requested arrays of `out` advanced to that row, K elements per row
// (rtx_query_hits: max_hits); null = not requested.  K == 0 is a count-only call: no targets, and `out` is not read
static DevQuery query_targets(uint32_t channels, const rtx_query_buffers * out, int64_t first, int64_t K = 1) {
    DevQuery t = {};
    if (K == 0) return t;
    auto at = [&](uint32_t bit, auto * array, int width) { return (channels & bit) && array ? array + width * K * first : nullptr; };
    t.distance = at(RTX_QUERY_DISTANCE, out->distance, 1);
    t.position = at(RTX_QUERY_POSITION, out->position, 3);
    t.normal = at(RTX_QUERY_NORMAL, out->normal, 3);
    t.uv = at(RTX_QUERY_UV, out->uv, 2);
    t.material_id = at(RTX_QUERY_MATERIAL_ID, out->material_id, 1);
    t.object_id = at(RTX_QUERY_OBJECT_ID, out->object_id, 1);
    t.triangle_id = at(RTX_QUERY_TRIANGLE_ID, out->triangle_id, 1);
    return t;
}
// the grid of a fill: the m rows of a round rounded up to whole packets
static dim3 query_fill_grid(int m) { return dim3((((m + RTX_WAVE - 1) & ~(RTX_WAVE - 1)) + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK); }

// One closest-hit round: the m rays at rays6 (device, 6 floats each) -> the hit records of slots [0, m) of level 1.  The caller reads them.
static int query_closest_round(rtx_ctx * c, const QueryCall & k, const float * rays6, int m) {
    if (k.order) if (int rc = query_sort_round<6>(c, k.S, rays6, m)) return rc;
    begin_batch(c, k.q.counters, k.q.pk_heads, 0u, false, true);
    launch_timed(c, "k_query_fill", c->stream, [&] { hipLaunchKernelGGL(k_query_fill, query_fill_grid(m), dim3(RTX_QUERY_BLOCK), 0, c->stream, k.q, rays6, m, k.order); });
    launch_timed(c, "k_trace_closest", c->stream, [&] { launch_closest_level1(c, k.sc, k.q, k.lane); });
    return RTX_OK;
}

// One occlusion round: the m segments at segments7 (device, 7 floats each) through ONE explicit shadow segment of level 0, whatever lights
// the frame has (none are read), then occluded[row] = 1 / 0.
static int query_occluded_round(rtx_ctx * c, const QueryCall & k, const float * segments7, int m, int32_t * occluded) {
    DevQueues q = k.q; q.shadow_explicit = 1;
    DevScene sc = k.sc; sc.light_count = 1;
    if (k.order) if (int rc = query_sort_round<7>(c, k.S, segments7, m)) return rc;
    begin_batch(c, q.counters, q.pk_heads, 0u, false, true);
    launch_timed(c, "k_query_fill_segments", c->stream, [&] { hipLaunchKernelGGL(k_query_fill_segments, query_fill_grid(m), dim3(RTX_QUERY_BLOCK), 0, c->stream, q, segments7, m, k.order); });
    launch_timed(c, "k_trace_any", c->stream, [&] { launch_any_level0(c, sc, q, k.lane); });
    launch_timed(c, "k_query_store_occluded", c->stream, [&] { hipLaunchKernelGGL(k_query_store_occluded, dim3((m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK), dim3(RTX_QUERY_BLOCK), 0, c->stream, q, m, occluded, k.order); });
    return RTX_OK;
}

extern "C" int rtx_query_closest(rtx_ctx * c, const void * rays_dev, int64_t n, uint32_t channels, const rtx_query_buffers * out, uint32_t flags) {
    if (c && (channels == 0 || (channels & ~(uint32_t)RTX_QUERY_ALL))) { c->err = "rtx_query_closest: channels must be a non-empty subset of RTX_QUERY_ALL"; return RTX_ERR_INVALID_ARG; }
    QueryCall k;
    if (int rc = query_setup(c, rays_dev, n, out, flags, "rtx_query_closest", k)) return rc;
    DevScene sc_resolve = k.sc; sc_resolve.diff_enabled = 0;        // the differentials are zero and no channel reports a RayHit differential
    return query_rounds(c, &k.q, n, [&](int64_t first, int m) -> int {
        const DevQuery t = query_targets(channels, out, first);
        if (int rc = query_closest_round(c, k, (const float *)rays_dev + 6 * first, m)) return rc;
        launch_timed(c, "k_query_resolve", c->stream, [&] { hipLaunchKernelGGL(k_query_resolve, dim3((m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK), dim3(RTX_QUERY_BLOCK), 0, c->stream, sc_resolve, k.q, m, t, k.order); });
        return RTX_OK;
    });
}

extern "C" int rtx_query_occluded(rtx_ctx * c, const void * segments_dev, int64_t n, int32_t * occluded_dev, uint32_t flags) {
    QueryCall k;
    if (int rc = query_setup(c, segments_dev, n, occluded_dev, flags, "rtx_query_occluded", k)) return rc;
    return query_rounds(c, &k.q, n, [&](int64_t first, int m) { return query_occluded_round(c, k, (const float *)segments_dev + 7 * first, m, occluded_dev + first); });
}

// the grid limit of the walk queries (k_query_nearest, k_query_hits, k_query_sweep, k_query_overlap): the spill regions are indexed by the global thread id;
// RTX_QUERY_GRID lowers it, so that a workgroup walks several tiles of a small call
static int query_max_blocks(const rtx_ctx * c) {
    const int fit = c->q.spill_threads / RTX_QUERY_BLOCK;
    return c->query_grid > 0 && c->query_grid < fit ? c->query_grid : fit;
}

// ---- object masks (include/rtx.h: rtx_set_object_masks ...; the rule is FILTER of rtx_nearest_math.h) -----------------------------------
// The table is the context's: M = I + S + P uint32_t in the numbering of RTX_AOV_OBJECT_ID, grown only (the one branch that waits), filled by
// a copy on the context's stream, so a query queued before a change reads the old masks and one queued after it the new ones.  Dropping the
// table keeps its memory.  The filtered queries take the pointer by value; rtx_set_frame, rtx_update_instances, refit and build never touch it.
static int32_t frame_object_count(const rtx_ctx * c) { return c->scene.instance_count + c->scene.sphere_count + c->scene.plane_count; }
static int object_mask_checks(rtx_ctx * c, const void * masks, int32_t count, const char * what, bool & drop) {
    if (!c) return RTX_ERR_INVALID_ARG;
    if (!c->frame_set) { c->err = std::string(what) + " before rtx_set_frame"; return RTX_ERR_STATE; }
    drop = !masks && count == 0;
    if (drop) return RTX_OK;
    if (!masks || count != frame_object_count(c)) {
        c->err = std::string(what) + ": count must be instances + spheres + planes of the current frame (" + std::to_string(frame_object_count(c)) + "), or 0 with a null pointer to drop the table";
        return RTX_ERR_INVALID_ARG;
    }
    return RTX_OK;
}
static int object_mask_room(rtx_ctx * c, size_t bytes) {
    if (bytes <= c->d_object_masks.cap && c->d_object_masks.p) return RTX_OK;
    HIP_OK(c, hipStreamSynchronize(c->stream));                // growth: queued queries still read the old table
    return ensure(c, c->d_object_masks, bytes);
}
static void object_masks_remember(rtx_ctx * c) {
    c->masks_set = true;
    c->mask_counts[0] = c->scene.instance_count; c->mask_counts[1] = c->scene.sphere_count; c->mask_counts[2] = c->scene.plane_count;
}
extern "C" int rtx_set_object_masks(rtx_ctx * c, const uint32_t * masks_host, int32_t count) {
    bool drop = false;
    if (int bad = object_mask_checks(c, masks_host, count, "rtx_set_object_masks", drop)) return bad;
    if (drop) { c->masks_set = false; return RTX_OK; }
    hipSetDevice(c->cfg.device);
    const size_t bytes = (size_t)count * sizeof(uint32_t);
    if (int rc = object_mask_room(c, bytes)) return rc;
    if (bytes) if (int rc = stage_copy(c, c->mask_ring, c->d_object_masks.p, masks_host, bytes)) return rc;
    object_masks_remember(c);
    return RTX_OK;
}
extern "C" int rtx_update_object_masks(rtx_ctx * c, const void * masks_dev, int32_t count) {
    bool drop = false;
    if (int bad = object_mask_checks(c, masks_dev, count, "rtx_update_object_masks", drop)) return bad;
    if (drop) { c->masks_set = false; return RTX_OK; }
    if ((uintptr_t)masks_dev & 3u) { c->err = "rtx_update_object_masks: the masks must be 4-byte aligned"; return RTX_ERR_INVALID_ARG; }
    hipSetDevice(c->cfg.device);
    const size_t bytes = (size_t)count * sizeof(uint32_t);
    if (int rc = object_mask_room(c, bytes)) return rc;
    if (bytes) HIP_OK(c, hipMemcpyAsync(c->d_object_masks.p, masks_dev, bytes, hipMemcpyDeviceToDevice, c->stream));
    object_masks_remember(c);
    return RTX_OK;
}
extern "C" int rtx_read_object_masks(rtx_ctx * c, uint32_t * out, int32_t capacity, int32_t * count) {
    if (!c || capacity < 0 || (!out && !count)) return RTX_ERR_INVALID_ARG;
    if (!c->frame_set) { c->err = "rtx_read_object_masks before rtx_set_frame"; return RTX_ERR_STATE; }
    const int32_t have = c->masks_set ? c->mask_counts[0] + c->mask_counts[1] + c->mask_counts[2] : 0;
    if (count) *count = have;
    if (!out || have == 0) return RTX_OK;
    if (capacity < have) { c->err = "rtx_read_object_masks: capacity below the table's " + std::to_string(have) + " masks"; return RTX_ERR_INVALID_ARG; }
    hipSetDevice(c->cfg.device);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    HIP_OK(c, hipMemcpy(out, c->d_object_masks.p, (size_t)have * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RTX_OK;
}
// the state rule of a filtered query, after the checks of the unfiltered call: a table set for other counts than the frame's
static int filter_checks(rtx_ctx * c, const rtx_query_filter * filter, const char * what) {
    if (!filter || !c->masks_set) return RTX_OK;
    if (c->mask_counts[0] != c->scene.instance_count || c->mask_counts[1] != c->scene.sphere_count || c->mask_counts[2] != c->scene.plane_count) {
        c->err = std::string(what) + "_filtered: the object masks were set for " + std::to_string(c->mask_counts[0]) + " instances, " + std::to_string(c->mask_counts[1]) + " spheres and " +
                 std::to_string(c->mask_counts[2]) + " planes, the frame has other counts (set the masks again, or drop them)";
        return RTX_ERR_STATE;
    }
    return RTX_OK;
}
// the kernel arguments of a filtered round that starts at caller row `first`
static QueryMasks<true> filter_masks(const rtx_ctx * c, const rtx_query_filter * filter, int64_t first) {
    QueryMasks<true> k;
    k.table = c->masks_set ? (const uint32_t *)c->d_object_masks.p : nullptr;
    k.rows = filter->row_masks_dev ? filter->row_masks_dev + first : nullptr;
    k.row = filter->row_mask;
    return k;
}

// ---- the walk queries' frame on the host: rtx_query_nearest / _signed_distance / _hits / _sweep / _overlap (kernels' frame: rtx_nearest.h) --
// n rows in device memory against the frame the context holds: per round of at most RTX_QUERY_CHUNK_RAYS rows ONE launch of the call's
// kernel, which reads the rows and writes the outputs; with RTX_QUERY_SORT the bounds, key and sort launches of the ray queries run first over
// the rows' key floats, in the same sort block.  No queue set, no counters: nothing a render call or rtx_get_stats reads is touched.  The
// stack lives in LDS and in the context's spill buffer, as for a closest-hit launch of this stream; all calls share one tile counter (they
// are ordered by the stream).
// The stack rule: a descent holds at most rtxnp::stack_need(TLAS inner depth, deepest BLAS inner depth) entries; a scene that needs more than
// rtx_config.stack_size (itself <= RTX_MAX_STACK, what LDS and the spill region hold per lane) is refused here, on the host.
// What a call decides once for all its rounds: the sort block and the sorted keys of a round (order; null = the caller's order), the tile
// counter (head; null only for rtx_query_nearest under RTX_NEAREST_FETCH=0), the scene by value, the spill buffer and the grid limit it sets, the filter (null: none).
struct WalkCall { QuerySort S; const uint64_t * order; uint32_t * head; DevScene sc; int32_t * spill; int spill_threads, max_blocks; const rtx_query_filter * filter; };
// after the call's own argument checks and query_checks, in this order: the rigid rule of the length queries (lengths: every walk query
// but rtx_query_hits, whose t is invariant under an affine map), the stack rule, the filter's state rule, then what allocates
// (rtx_query_signed_distance brings its side tables up to date behind it: side_table_current, which allocates and queues a copy, now
// follows the tile counter's allocation; before, it came between the sort block and the counter)
static int walk_setup(rtx_ctx * c, const char * what, const char * descent_word, int64_t n, uint32_t flags, const rtx_query_filter * filter, WalkCall & k, bool lengths, bool counter = true) {
    if (lengths && !c->frame_rigid) {
        c->err = std::string(what) + ": the frame holds an instance whose world / world_inv is not a rigid pose (scaled, sheared or flattened); the walk prunes by world-space distances and would miss answers";
        return RTX_ERR_STATE;
    }
    int blas_depth = -1;
    for (size_t b = 0; b < c->blas.size(); b++) if (c->h_blas[b].nodes && c->blas[b].inner_depth > blas_depth) blas_depth = c->blas[b].inner_depth;
    const int need = rtxnp::stack_need(c->tlas_inner_depth, blas_depth), have = c->cfg.stack_size < RTX_MAX_STACK ? c->cfg.stack_size : RTX_MAX_STACK;
    if (need > have) {
        c->err = std::string(what) + ": the " + descent_word + " needs " + std::to_string(need) + " stack entries (TLAS inner depth " + std::to_string(c->tlas_inner_depth) +
                 " + 1, BLAS inner depth " + std::to_string(blas_depth) + " + 1), rtx_config.stack_size allows " + std::to_string(have);
        return RTX_ERR_LIMIT;
    }
    if (int bad = filter_checks(c, filter, what)) return bad;
    hipSetDevice(c->cfg.device);
    k.S = {};
    k.order = nullptr;
    if (flags & RTX_QUERY_SORT) {
        if (int rc = query_queues(c, n, nullptr, &k.S)) return rc;
        k.order = k.S.keys;
    }
    if (counter) if (int rc = ensure(c, c->d_nearest_head, sizeof(uint32_t))) return rc;      // the first call only
    k.head = counter ? (uint32_t *)c->d_nearest_head.p : nullptr;
    k.sc = c->scene;
    k.spill = (int32_t *)c->d_spill.p; k.spill_threads = c->q.spill_threads;
    k.max_blocks = query_max_blocks(c);
    k.filter = filter;
    return RTX_OK;
}
// The rounds of a walk query over n rows of ROW floats (sort key: the first KEY): the sort, the grid and the counter's reset of every round,
// then launch(first, rows, m, blocks) for the one kernel launch over rows [first, first + m) at `rows`
template <int ROW, int KEY = ROW, typename F> static int walk_rounds(rtx_ctx * c, const WalkCall & k, const void * rows_dev, int64_t n, F && launch) {
    return query_rounds(c, nullptr, n, [&](int64_t first, int m) -> int {
        const float * const rows = (const float *)rows_dev + ROW * first;
        if (k.order) if (int rc = query_sort_round<ROW, KEY>(c, k.S, rows, m)) return rc;
        const int tiles = (m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK, blocks = tiles < k.max_blocks ? tiles : k.max_blocks;
        if (k.head) HIP_OK(c, hipMemsetAsync(k.head, 0, sizeof(uint32_t), c->stream));
        launch(first, rows, m, blocks);
        return RTX_OK;
    });
}
// The launch of the round that starts at caller row `first`, timed as `name`: kernel(masks) launches the instantiation for the type of
// masks (its ::filtered is the template argument) — QueryMasks<true>, the filter's masks from that row on, or QueryMasks<false>
template <typename Launch> static void walk_launch(rtx_ctx * c, const WalkCall & k, const char * name, int64_t first, Launch && kernel) {
    launch_timed(c, name, c->stream, [&] {
        if (k.filter) kernel(filter_masks(c, k.filter, first));
        else kernel(QueryMasks<false>());
    });
}

// ---- nearest-point queries (include/rtx.h: rtx_query_nearest; kernel in rtx_nearest.h, arithmetic and walk in rtx_nearest_math.h) ------
// The walk queries' frame over n points with a maximum distance each: k_query_nearest writes the channels; the sort key is the 4-float row.
// rtx_query_signed_distance is the same call with two more outputs (sg: signed_dev [n], feature_dev [n] or null) and the SIGNED
// instantiations; its channels may be empty, and then out may be null.
struct QuerySigned { float * signed_dev; int32_t * feature_dev; };
// the device copy of h_side covers every BLAS id and is current: growth waits for the stream (queued signed queries read the old table), an
// update is a staged copy on the stream, a steady-state call does neither
static int side_table_current(rtx_ctx * c) {
    const size_t ids = c->h_blas.size(), bytes = ids * sizeof(DevSideBlas);
    if (c->h_side.size() < ids) { DevSideBlas none; memset(&none, 0, sizeof(none)); c->h_side.resize(ids, none); c->side_dirty = true; }
    if (!c->d_side.p || bytes > c->d_side.cap) {
        DevBuf nb;
        if (int rc = ensure(c, nb, bytes)) return rc;
        HIP_OK(c, hipStreamSynchronize(c->stream));
        c->d_side = std::move(nb);
        c->side_dirty = true;
    }
    if (c->side_dirty && bytes) if (int rc = stage_copy(c, c->side_ring, c->d_side.p, c->h_side.data(), bytes)) return rc;
    c->side_dirty = false;
    return RTX_OK;
}
static int query_nearest_impl(rtx_ctx * c, const void * points_dev, int64_t n, uint32_t channels, const rtx_query_buffers * out, uint32_t flags, const rtx_query_filter * filter,
                              const QuerySigned * sg = nullptr) {
    const char * const what = sg ? "rtx_query_signed_distance" : "rtx_query_nearest";
    if (c && sg) {
        if (channels & ~(uint32_t)RTX_QUERY_ALL) { c->err = "rtx_query_signed_distance: channels must be a subset of RTX_QUERY_ALL"; return RTX_ERR_INVALID_ARG; }
        if (!sg->signed_dev || (((uintptr_t)sg->signed_dev | (uintptr_t)sg->feature_dev) & 3)) { c->err = "rtx_query_signed_distance: null or misaligned signed-distance or feature pointer"; return RTX_ERR_INVALID_ARG; }
        static const rtx_query_buffers no_buffers = {};
        if (channels == 0 && !out) out = &no_buffers;                  // no channel bit is set: nothing of it is read
    } else if (c && (channels == 0 || (channels & ~(uint32_t)RTX_QUERY_ALL))) { c->err = "rtx_query_nearest: channels must be a non-empty subset of RTX_QUERY_ALL"; return RTX_ERR_INVALID_ARG; }
    if (int bad = query_checks(c, points_dev, n, out, flags, what, (uint32_t)RTX_QUERY_SORT)) return bad;
    WalkCall k;
    if (int rc = walk_setup(c, what, "ordered descent", n, flags, filter, k, true, c->nearest_fetch)) return rc;
    if (sg) if (int rc = side_table_current(c)) return rc;
    return walk_rounds<4>(c, k, points_dev, n, [&](int64_t first, const float * rows, int m, int blocks) {
        const DevQuery t = query_targets(channels, out, first);
        QuerySide<true> ks = { nullptr, nullptr, nullptr };
        if (sg) { ks.blas = (const DevSideBlas *)c->d_side.p; ks.signed_out = sg->signed_dev + first; ks.feature = sg->feature_dev ? sg->feature_dev + first : nullptr; }
        walk_launch(c, k, "k_query_nearest", first, [&](auto km) {
            auto go = [&](auto side) {
                hipLaunchKernelGGL((k_query_nearest<decltype(km)::filtered, decltype(side)::is_signed>), dim3(blocks), dim3(RTX_QUERY_BLOCK), 0, c->stream,
                                   k.sc, rows, m, t, k.order, k.spill, k.spill_threads, k.head, km, side);
            };
            if (sg) go(ks); else go(QuerySide<false>());
        });
    });
}
extern "C" int rtx_query_nearest(rtx_ctx * c, const void * points_dev, int64_t n, uint32_t channels, const rtx_query_buffers * out, uint32_t flags) {
    return query_nearest_impl(c, points_dev, n, channels, out, flags, nullptr);
}
extern "C" int rtx_query_nearest_filtered(rtx_ctx * c, const void * points_dev, int64_t n, uint32_t channels, const rtx_query_buffers * out, uint32_t flags, const rtx_query_filter * filter) {
    return query_nearest_impl(c, points_dev, n, channels, out, flags, filter);
}
extern "C" int rtx_query_signed_distance(rtx_ctx * c, const void * points_dev, int64_t n, uint32_t channels, const rtx_query_buffers * out,
                                         float * signed_dev, int32_t * feature_dev, uint32_t flags, const rtx_query_filter * filter) {
    const QuerySigned sg = { signed_dev, feature_dev };
    return query_nearest_impl(c, points_dev, n, channels, out, flags, filter, &sg);
}

// ---- all-hits segment queries (include/rtx.h: rtx_query_hits; kernel in rtx_hits.h, arithmetic and walk in rtx_hits_math.h) ------------
// The walk queries' frame over n segments: k_query_hits writes the first max_hits hits of every row, in order, and the row's count; the sort
// key is the 7-float row.
static int query_hits_impl(rtx_ctx * c, const void * segments_dev, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                           int32_t * count_dev, uint32_t flags, const rtx_query_filter * filter) {
    if (c) {
        const bool count_only = max_hits == 0 && channels == 0 && count_dev;
        if (!count_only && (max_hits < 1 || max_hits > (int32_t)RTX_QUERY_MAX_HITS || channels == 0 || (channels & ~(uint32_t)RTX_QUERY_ALL))) {
            c->err = "rtx_query_hits: max_hits must be in [1, RTX_QUERY_MAX_HITS] with channels a non-empty subset of RTX_QUERY_ALL, or max_hits == 0 and channels == 0 with a count_dev";
            return RTX_ERR_INVALID_ARG;
        }
    }
    if (int bad = query_checks(c, segments_dev, n, max_hits ? (const void *)out : (const void *)count_dev, flags, "rtx_query_hits", (uint32_t)RTX_QUERY_SORT)) return bad;
    WalkCall k;
    if (int rc = walk_setup(c, "rtx_query_hits", "ordered descent", n, flags, filter, k, false)) return rc;
    const int64_t K = max_hits;
    return walk_rounds<7>(c, k, segments_dev, n, [&](int64_t first, const float * rows, int m, int blocks) {
        const DevQuery t = query_targets(channels, out, first, K);
        int32_t * const count = count_dev ? count_dev + first : nullptr;
        walk_launch(c, k, "k_query_hits", first, [&](auto km) {
            auto go = [&](auto list) {
                hipLaunchKernelGGL((k_query_hits<decltype(list)::value, decltype(km)::filtered>), dim3(blocks), dim3(RTX_QUERY_BLOCK), 0, c->stream,
                                   k.sc, rows, m, (int)K, t, count, k.order, k.spill, k.spill_threads, k.head, km);
            };
            if (K > 0) go(std::true_type()); else go(std::false_type());
        });
    });
}
extern "C" int rtx_query_hits(rtx_ctx * c, const void * segments_dev, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                              int32_t * count_dev, uint32_t flags) {
    return query_hits_impl(c, segments_dev, n, max_hits, channels, out, count_dev, flags, nullptr);
}
extern "C" int rtx_query_hits_filtered(rtx_ctx * c, const void * segments_dev, int64_t n, int32_t max_hits, uint32_t channels, const rtx_query_buffers * out,
                                       int32_t * count_dev, uint32_t flags, const rtx_query_filter * filter) {
    return query_hits_impl(c, segments_dev, n, max_hits, channels, out, count_dev, flags, filter);
}

// ---- swept-sphere queries (include/rtx.h: rtx_query_sweep; kernel in rtx_sweep.h, arithmetic and walk in rtx_sweep_math.h) ------------
// The walk queries' frame over n sweeps: k_query_sweep writes the channels; the sort key is the first seven floats of the 8-float rows.
static int query_sweep_impl(rtx_ctx * c, const void * sweeps_dev, int64_t n, uint32_t channels, const rtx_query_buffers * out, uint32_t flags, const rtx_query_filter * filter) {
    if (c && (channels == 0 || (channels & ~(uint32_t)RTX_QUERY_ALL))) { c->err = "rtx_query_sweep: channels must be a non-empty subset of RTX_QUERY_ALL"; return RTX_ERR_INVALID_ARG; }
    if (int bad = query_checks(c, sweeps_dev, n, out, flags, "rtx_query_sweep", (uint32_t)RTX_QUERY_SORT)) return bad;
    WalkCall k;
    if (int rc = walk_setup(c, "rtx_query_sweep", "ordered descent", n, flags, filter, k, true)) return rc;
    return walk_rounds<8, 7>(c, k, sweeps_dev, n, [&](int64_t first, const float * rows, int m, int blocks) {
        const DevQuery t = query_targets(channels, out, first);
        walk_launch(c, k, "k_query_sweep", first, [&](auto km) {
            hipLaunchKernelGGL((k_query_sweep<decltype(km)::filtered>), dim3(blocks), dim3(RTX_QUERY_BLOCK), 0, c->stream,
                               k.sc, rows, m, t, k.order, k.spill, k.spill_threads, k.head, km);
        });
    });
}
extern "C" int rtx_query_sweep(rtx_ctx * c, const void * sweeps_dev, int64_t n, uint32_t channels, const rtx_query_buffers * out, uint32_t flags) {
    return query_sweep_impl(c, sweeps_dev, n, channels, out, flags, nullptr);
}
extern "C" int rtx_query_sweep_filtered(rtx_ctx * c, const void * sweeps_dev, int64_t n, uint32_t channels, const rtx_query_buffers * out, uint32_t flags, const rtx_query_filter * filter) {
    return query_sweep_impl(c, sweeps_dev, n, channels, out, flags, filter);
}

// ---- box-overlap queries (include/rtx.h: rtx_query_overlap; kernel in rtx_overlap.h, arithmetic and walk in rtx_overlap_math.h) ---------
// The walk queries' frame over n boxes: k_query_overlap writes the ids of the max_hits smallest overlaps of every row and the row's count.
// The sort key is the first four floats of the 10-float rows — the position key of rtx_query_nearest; its fourth float is h.x here, so a box
// with h.x == 0 sorts with the dead rows, last, and is walked all the same.  The stack uses region 0 of the spill buffer only.
static int query_overlap_impl(rtx_ctx * c, const void * boxes_dev, int64_t n, int32_t max_hits, int32_t * object_id_dev, int32_t * triangle_id_dev, int32_t * count_dev,
                              uint32_t flags, const rtx_query_filter * filter) {
    const bool any = (flags & RTX_OVERLAP_ANY) != 0, objects = (flags & RTX_OVERLAP_OBJECTS) != 0;
    if (c) {
        const char * bad = nullptr;
        if (max_hits < 0 || max_hits > (int32_t)RTX_QUERY_MAX_HITS) bad = "max_hits must be in [0, RTX_QUERY_MAX_HITS]";
        else if (any && (max_hits != 0 || objects)) bad = "RTX_OVERLAP_ANY needs max_hits == 0 and excludes RTX_OVERLAP_OBJECTS";
        else if (objects && triangle_id_dev) bad = "RTX_OVERLAP_OBJECTS reports no triangle ids: triangle_id_dev must be NULL";
        else if (max_hits == 0 && !count_dev) bad = "max_hits == 0 is the count-only form (or RTX_OVERLAP_ANY) and needs a count_dev";
        else if (max_hits > 0 && !object_id_dev && !triangle_id_dev) bad = "max_hits > 0 needs object_id_dev or triangle_id_dev";
        if (bad) { c->err = std::string("rtx_query_overlap: ") + bad; return RTX_ERR_INVALID_ARG; }
    }
    const void * const some_out = object_id_dev ? (const void *)object_id_dev : triangle_id_dev ? (const void *)triangle_id_dev : (const void *)count_dev;
    if (int bad = query_checks(c, boxes_dev, n, some_out, flags, "rtx_query_overlap", (uint32_t)RTX_QUERY_SORT | (uint32_t)RTX_OVERLAP_OBJECTS | (uint32_t)RTX_OVERLAP_ANY)) return bad;
    WalkCall k;
    if (int rc = walk_setup(c, "rtx_query_overlap", "descent", n, flags, filter, k, true)) return rc;
    const int64_t K = max_hits;
    return walk_rounds<rtxop::ROW_FLOATS, 4>(c, k, boxes_dev, n, [&](int64_t first, const float * rows, int m, int blocks) {
        int32_t * const count = count_dev ? count_dev + first : nullptr;
        // the kernel of form `form` with list length `held` (0: no list, and no ids); triangle ids only where the form reports them
        auto go = [&](auto form, int held, bool triangles) {
            int32_t * const object_id = held && object_id_dev ? object_id_dev + K * first : nullptr;
            int32_t * const triangle_id = held && triangles && triangle_id_dev ? triangle_id_dev + K * first : nullptr;
            walk_launch(c, k, "k_query_overlap", first, [&](auto km) {
                hipLaunchKernelGGL((k_query_overlap<decltype(form)::value, decltype(km)::filtered>), dim3(blocks), dim3(RTX_QUERY_BLOCK), 0, c->stream,
                                   k.sc, rows, m, held, object_id, triangle_id, count, k.order, k.spill, k.spill_threads, k.head, km);
            });
        };
        if (any) go(std::integral_constant<int, rtxop::FORM_ANY>(), 0, false);
        else if (objects && K > 0) go(std::integral_constant<int, rtxop::FORM_OBJECTS>(), (int)K, false);
        else if (objects) go(std::integral_constant<int, rtxop::FORM_OBJECTS | OVERLAP_COUNT_ONLY>(), 0, false);
        else if (K > 0) go(std::integral_constant<int, rtxop::FORM_TRIANGLES>(), (int)K, true);
        else go(std::integral_constant<int, rtxop::FORM_TRIANGLES | OVERLAP_COUNT_ONLY>(), 0, false);
    });
}
extern "C" int rtx_query_overlap(rtx_ctx * c, const void * boxes_dev, int64_t n, int32_t max_hits, int32_t * object_id_dev, int32_t * triangle_id_dev, int32_t * count_dev, uint32_t flags) {
    return query_overlap_impl(c, boxes_dev, n, max_hits, object_id_dev, triangle_id_dev, count_dev, flags, nullptr);
}
extern "C" int rtx_query_overlap_filtered(rtx_ctx * c, const void * boxes_dev, int64_t n, int32_t max_hits, int32_t * object_id_dev, int32_t * triangle_id_dev, int32_t * count_dev,
                                          uint32_t flags, const rtx_query_filter * filter) {
    return query_overlap_impl(c, boxes_dev, n, max_hits, object_id_dev, triangle_id_dev, count_dev, flags, filter);
}

// ---- capsule-overlap queries (include/rtx.h: rtx_query_overlap_capsule; kernel in rtx_capsule.h, arithmetic and walk in rtx_capsule_math.h) --
// rtx_query_overlap's call over n capsules of seven floats.  The sort key is the ray key over the first six floats (start point, axis), so a
// ball row (axis 0) sorts with the dead rows, last, and is walked all the same.  The stack uses region 0 of the spill buffer only.
static int query_overlap_capsule_impl(rtx_ctx * c, const void * capsules_dev, int64_t n, int32_t max_hits, int32_t * object_id_dev, int32_t * triangle_id_dev, int32_t * count_dev,
                                      uint32_t flags, const rtx_query_filter * filter) {
    const bool any = (flags & RTX_OVERLAP_ANY) != 0, objects = (flags & RTX_OVERLAP_OBJECTS) != 0;
    if (c) {
        const char * bad = nullptr;
        if (max_hits < 0 || max_hits > (int32_t)RTX_QUERY_MAX_HITS) bad = "max_hits must be in [0, RTX_QUERY_MAX_HITS]";
        else if (any && (max_hits != 0 || objects)) bad = "RTX_OVERLAP_ANY needs max_hits == 0 and excludes RTX_OVERLAP_OBJECTS";
        else if (objects && triangle_id_dev) bad = "RTX_OVERLAP_OBJECTS reports no triangle ids: triangle_id_dev must be NULL";
        else if (max_hits == 0 && !count_dev) bad = "max_hits == 0 is the count-only form (or RTX_OVERLAP_ANY) and needs a count_dev";
        else if (max_hits > 0 && !object_id_dev && !triangle_id_dev) bad = "max_hits > 0 needs object_id_dev or triangle_id_dev";
        if (bad) { c->err = std::string("rtx_query_overlap_capsule: ") + bad; return RTX_ERR_INVALID_ARG; }
    }
    const void * const some_out = object_id_dev ? (const void *)object_id_dev : triangle_id_dev ? (const void *)triangle_id_dev : (const void *)count_dev;
    if (int bad = query_checks(c, capsules_dev, n, some_out, flags, "rtx_query_overlap_capsule", (uint32_t)RTX_QUERY_SORT | (uint32_t)RTX_OVERLAP_OBJECTS | (uint32_t)RTX_OVERLAP_ANY)) return bad;
    WalkCall k;
    if (int rc = walk_setup(c, "rtx_query_overlap_capsule", "descent", n, flags, filter, k, true)) return rc;
    const int64_t K = max_hits;
    return walk_rounds<rtxcp::ROW_FLOATS, rtxcp::KEY_FLOATS>(c, k, capsules_dev, n, [&](int64_t first, const float * rows, int m, int blocks) {
        int32_t * const count = count_dev ? count_dev + first : nullptr;
        auto go = [&](auto form, int held, bool triangles) {
            int32_t * const object_id = held && object_id_dev ? object_id_dev + K * first : nullptr;
            int32_t * const triangle_id = held && triangles && triangle_id_dev ? triangle_id_dev + K * first : nullptr;
            walk_launch(c, k, "k_query_overlap_capsule", first, [&](auto km) {
                hipLaunchKernelGGL((k_query_overlap_capsule<decltype(form)::value, decltype(km)::filtered>), dim3(blocks), dim3(RTX_QUERY_BLOCK), 0, c->stream,
                                   k.sc, rows, m, held, object_id, triangle_id, count, k.order, k.spill, k.spill_threads, k.head, km);
            });
        };
        if (any) go(std::integral_constant<int, rtxcp::FORM_ANY>(), 0, false);
        else if (objects && K > 0) go(std::integral_constant<int, rtxcp::FORM_OBJECTS>(), (int)K, false);
        else if (objects) go(std::integral_constant<int, rtxcp::FORM_OBJECTS | OVERLAP_COUNT_ONLY>(), 0, false);
        else if (K > 0) go(std::integral_constant<int, rtxcp::FORM_TRIANGLES>(), (int)K, true);
        else go(std::integral_constant<int, rtxcp::FORM_TRIANGLES | OVERLAP_COUNT_ONLY>(), 0, false);
    });
}
extern "C" int rtx_query_overlap_capsule(rtx_ctx * c, const void * capsules_dev, int64_t n, int32_t max_hits, int32_t * object_id_dev, int32_t * triangle_id_dev, int32_t * count_dev, uint32_t flags) {
    return query_overlap_capsule_impl(c, capsules_dev, n, max_hits, object_id_dev, triangle_id_dev, count_dev, flags, nullptr);
}
extern "C" int rtx_query_overlap_capsule_filtered(rtx_ctx * c, const void * capsules_dev, int64_t n, int32_t max_hits, int32_t * object_id_dev, int32_t * triangle_id_dev, int32_t * count_dev,
                                                  uint32_t flags, const rtx_query_filter * filter) {
    return query_overlap_capsule_impl(c, capsules_dev, n, max_hits, object_id_dev, triangle_id_dev, count_dev, flags, filter);
}

// ---- swept-box queries (include/rtx.h: rtx_query_sweep_box; kernel in rtx_boxsweep.h, arithmetic and walk in rtx_boxsweep_math.h) -------
// The walk queries' frame over n sweeps: k_query_sweep_box writes t, the normal, the ids and the axis code; the sort key is the first seven
// floats of the 14-float rows, the ray key of rtx_query_sweep.
static int query_sweep_box_impl(rtx_ctx * c, const void * sweeps_dev, int64_t n, float * t_dev, float * normal_dev, int32_t * object_id_dev, int32_t * triangle_id_dev, int32_t * axis_dev,
                                uint32_t flags, const rtx_query_filter * filter) {
    const void * const some_out = t_dev ? (const void *)t_dev : normal_dev ? (const void *)normal_dev : object_id_dev ? (const void *)object_id_dev :
                                  triangle_id_dev ? (const void *)triangle_id_dev : (const void *)axis_dev;
    if (int bad = query_checks(c, sweeps_dev, n, some_out, flags, "rtx_query_sweep_box", (uint32_t)RTX_QUERY_SORT)) return bad;
    WalkCall k;
    if (int rc = walk_setup(c, "rtx_query_sweep_box", "ordered descent", n, flags, filter, k, true)) return rc;
    return walk_rounds<rtxbs::ROW_FLOATS, rtxbs::KEY_FLOATS>(c, k, sweeps_dev, n, [&](int64_t first, const float * rows, int m, int blocks) {
        const DevBoxSweep t = { t_dev ? t_dev + first : nullptr, normal_dev ? normal_dev + 3 * first : nullptr, object_id_dev ? object_id_dev + first : nullptr,
                                triangle_id_dev ? triangle_id_dev + first : nullptr, axis_dev ? axis_dev + first : nullptr };
        walk_launch(c, k, "k_query_sweep_box", first, [&](auto km) {
            hipLaunchKernelGGL((k_query_sweep_box<decltype(km)::filtered>), dim3(blocks), dim3(RTX_QUERY_BLOCK), 0, c->stream,
                               k.sc, rows, m, t, k.order, k.spill, k.spill_threads, k.head, km);
        });
    });
}
extern "C" int rtx_query_sweep_box(rtx_ctx * c, const void * sweeps_dev, int64_t n, float * t_dev, float * normal_dev, int32_t * object_id_dev, int32_t * triangle_id_dev, int32_t * axis_dev, uint32_t flags) {
    return query_sweep_box_impl(c, sweeps_dev, n, t_dev, normal_dev, object_id_dev, triangle_id_dev, axis_dev, flags, nullptr);
}
extern "C" int rtx_query_sweep_box_filtered(rtx_ctx * c, const void * sweeps_dev, int64_t n, float * t_dev, float * normal_dev, int32_t * object_id_dev, int32_t * triangle_id_dev, int32_t * axis_dev,
                                            uint32_t flags, const rtx_query_filter * filter) {
    return query_sweep_box_impl(c, sweeps_dev, n, t_dev, normal_dev, object_id_dev, triangle_id_dev, axis_dev, flags, filter);
}

// the order RTX_QUERY_SORT traces n rows of row_floats (6: rays, 7: segments) floats in: the bounds, key and sort launches of every round and
// nothing else, order_out[first + i] = first + the row of slot i of the round that starts at `first`.  Queued like the queries; their checks.
extern "C" int rtx_debug_query_order(rtx_ctx * c, const void * rows_dev, int32_t row_floats, int64_t n, int32_t * order_out_dev) {
    if (int bad = query_checks(c, rows_dev, n, order_out_dev, 0u, "rtx_debug_query_order")) return bad;
    if (row_floats != 4 && row_floats != 6 && row_floats != 7) { c->err = "rtx_debug_query_order: row_floats must be 4, 6 or 7"; return RTX_ERR_INVALID_ARG; }
    if (n > (int64_t)INT32_MAX) { c->err = "rtx_debug_query_order: more rows than an int32_t order holds"; return RTX_ERR_LIMIT; }
    hipSetDevice(c->cfg.device);
    DevQueues q;
    QuerySort S;
    if (int rc = query_queues(c, n, &q, &S)) return rc;
    return query_rounds(c, &q, n, [&](int64_t first, int m) -> int {
        const float * const rows = (const float *)rows_dev + (size_t)row_floats * first;
        if (int rc = row_floats == 4 ? query_sort_round<4>(c, S, rows, m) : row_floats == 6 ? query_sort_round<6>(c, S, rows, m) : query_sort_round<7>(c, S, rows, m)) return rc;
        launch_timed(c, "k_query_sort_order", c->stream, [&] { hipLaunchKernelGGL(k_query_sort_order, dim3((m + RTX_QUERY_BLOCK - 1) / RTX_QUERY_BLOCK), dim3(RTX_QUERY_BLOCK), 0, c->stream, (const uint64_t *)S.keys, m, (int32_t)first, order_out_dev + first); });
        return RTX_OK;
    });
}

// ---- unit-level entry points, second set: the traversal / hit / light / plot functions at caller-supplied inputs -------------------
// rtx_debug_trace_rays: n rays (18 floats: origin, direction, dO_dx, dO_dy, dD_dx, dD_dy) from host memory through the closest-hit rounds of
// the ray queries above (query_setup, query_closest_round), then the accept-branch rebuild of k_shade with the rays' differentials: all
// RayHit fields out (27 floats, layout of oracle orc_trace_closest).  rtx_debug_occluded: n host segments through the queries' occlusion
// rounds.  Both wait and copy back.
// slots [0, m) of level 1 of a round -> out; the differentials come from the 18-float rows.  No hit (a miss, or a row the fill did not
// walk): hit 0, distance +INFINITY, every other float 0, as the oracle's miss record.
__global__ void k_debug_rebuild(DevScene sc, DevQueues q, const float * rays, float * out, int m) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const float * r = rays + 18 * (size_t)i;
    RayFull ray;
    ray.o = V3(r[0], r[1], r[2]); ray.d = V3(r[3], r[4], r[5]); ray.dO_dx = V3(r[6], r[7], r[8]); ray.dO_dy = V3(r[9], r[10], r[11]);
    ray.dD_dx = V3(r[12], r[13], r[14]); ray.dD_dy = V3(r[15], r[16], r[17]);
    const uint32_t s = (uint32_t)q.level_base[1] + (uint32_t)i;
    const float4 h0 = q.h0[s]; const int tri = q.h1[s], prim = as_i(h0.w);
    float * o = out + 27 * (size_t)i;
    for (int k = 0; k < 27; k++) o[k] = 0.0f;
    o[1] = INFINITY;
    if (PRIM_KIND(prim) == PRIM_NONE) return;
    HitFull h; h.material_id = 0;
    h.point = h.normal = h.dO_dx = h.dO_dy = h.dN_dx = h.dN_dy = V3(0, 0, 0); h.u = h.v = h.ds_dx = h.ds_dy = h.dt_dx = h.dt_dy = 0.0f;
    if (PRIM_KIND(prim) == PRIM_TRI) rebuild_triangle_hit(sc, PRIM_INDEX(prim), tri, h0.x, h0.y, h0.z, ray, h);
    else if (PRIM_KIND(prim) == PRIM_SPHERE) rebuild_sphere_hit(sc, sc.spheres[PRIM_INDEX(prim)], h0.x, ray, h);
    else rebuild_plane_hit(sc, sc.planes[PRIM_INDEX(prim)], h0.x, ray, h);
    o[0] = 1.0f; o[1] = h0.x; o[2] = h.point.x; o[3] = h.point.y; o[4] = h.point.z; o[5] = h.normal.x; o[6] = h.normal.y; o[7] = h.normal.z;
    o[8] = (float)h.material_id; o[9] = h.u; o[10] = h.v; o[11] = h.ds_dx; o[12] = h.ds_dy; o[13] = h.dt_dx; o[14] = h.dt_dy;
    o[15] = h.dO_dx.x; o[16] = h.dO_dx.y; o[17] = h.dO_dx.z; o[18] = h.dO_dy.x; o[19] = h.dO_dy.y; o[20] = h.dO_dy.z;
    o[21] = h.dN_dx.x; o[22] = h.dN_dx.y; o[23] = h.dN_dx.z; o[24] = h.dN_dy.x; o[25] = h.dN_dy.y; o[26] = h.dN_dy.z;
}

extern "C" int rtx_debug_trace_rays(rtx_ctx * c, const float * rays18, int32_t n, float * hits27, uint32_t flags) {
    if (!c) return RTX_ERR_INVALID_ARG;
    // bounces < 1: a plain argument check, kept from when the hook borrowed the frame's level-1 queue (no ray needs it); RTX_QUERY_SORT: slot i is row i here
    if (c->cfg.bounces < 1 || (flags & RTX_QUERY_SORT)) { c->err = "rtx_debug_trace_rays: bounces < 1 or RTX_QUERY_SORT"; return RTX_ERR_INVALID_ARG; }
    QueryCall k;
    if (int rc = query_setup(c, rays18, n, hits27, flags, "rtx_debug_trace_rays", k)) return rc;
    std::vector<float> rays6((size_t)n * 6);                        // the rows k_query_fill takes: origin and direction
    for (int32_t i = 0; i < n; i++) memcpy(&rays6[(size_t)i * 6], rays18 + (size_t)i * 18, 24);
    DevBuf din, din6, dout;
    int rc = upload(c, din, rays18, (size_t)n * 72);
    if (!rc) rc = upload(c, din6, rays6.data(), (size_t)n * 24);
    if (!rc) rc = ensure(c, dout, (size_t)n * 108);
    if (!rc) rc = query_rounds(c, &k.q, n, [&](int64_t first, int m) -> int {
        if (int bad = query_closest_round(c, k, (const float *)din6.p + 6 * first, m)) return bad;
        hipLaunchKernelGGL(k_debug_rebuild, dim3((m + 255) / 256), dim3(256), 0, c->stream, k.sc, k.q, (const float *)din.p + 18 * first, (float *)dout.p + 27 * first, m);
        return RTX_OK;
    });
    HIP_OK(c, hipStreamSynchronize(c->stream));                     // also on an error: what was queued reads the buffers that go out of scope here
    if (rc) return rc;
    HIP_OK(c, hipMemcpy(hits27, dout.p, (size_t)n * 108, hipMemcpyDeviceToHost));
    return RTX_OK;
}

extern "C" int rtx_debug_occluded(rtx_ctx * c, const float * origin_direction_maxdist7, int32_t n, uint32_t * occluded, uint32_t flags) {
    if (!c) return RTX_ERR_INVALID_ARG;
    // no light: a plain argument check, kept from when the hook borrowed light 0's shadow segment (no segment needs one); RTX_QUERY_SORT: refused as above
    if (c->scene.light_count < 1 || (flags & RTX_QUERY_SORT)) { c->err = "rtx_debug_occluded: a frame without lights or RTX_QUERY_SORT"; return RTX_ERR_INVALID_ARG; }
    QueryCall k;
    if (int rc = query_setup(c, origin_direction_maxdist7, n, occluded, flags, "rtx_debug_occluded", k)) return rc;
    DevBuf din, dout;
    int rc = upload(c, din, origin_direction_maxdist7, (size_t)n * 28);
    if (!rc) rc = ensure(c, dout, (size_t)n * 4);
    if (!rc) rc = query_rounds(c, &k.q, n, [&](int64_t first, int m) { return query_occluded_round(c, k, (const float *)din.p + 7 * first, m, (int32_t *)dout.p + first); });
    HIP_OK(c, hipStreamSynchronize(c->stream));
    if (rc) return rc;
    HIP_OK(c, hipMemcpy(occluded, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RTX_OK;
}

__global__ void k_debug_light_plot(rtx_point_light pl, rtx_spot_light sl, rtx_directional_light dl, const float * in10, float * out9, const float * rgb, uint32_t * packed, int n_light, int n_plot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_light) {
        const float * r = in10 + 10 * (size_t)i;
        const v3 nrm = V3(r[0], r[1], r[2]), tl = V3(r[3], r[4], r[5]), tc = V3(r[6], r[7], r[8]); const float d2 = r[9];
        const v3 a = vdivs(light_calc(v3p(pl.colour), nrm, tl, tc), d2);                      // PointLight.h:9-11
        v3 b = V3(0.0f, 0.0f, 0.0f);                                                           // SpotLight.h:17-33, as k_shade evaluates it
        const float dt = vdot(tl, v3p(sl.negative_direction));
        if (dt > sl.outer_cutoff) { float f = (dt - sl.outer_cutoff) / (sl.inner_cutoff - sl.outer_cutoff); f = (f > 1.0f) ? 1.0f : f; b = vmuls(vdivs(light_calc(v3p(sl.colour), nrm, tl, tc), d2), f); }
        const v3 cc = light_calc(v3p(dl.colour), nrm, v3p(dl.negative_direction), tc);         // DirectionalLight.h:9-11
        float * o = out9 + 9 * (size_t)i;
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = b.x; o[4] = b.y; o[5] = b.z; o[6] = cc.x; o[7] = cc.y; o[8] = cc.z;
    }
    if (i < n_plot) packed[i] = plot_pack(V3(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]));     // Window::plot, Window.h:56-65
}

// Light::calc_lighting of the three light kinds (k_shade's expressions) and Window::plot at caller-supplied inputs
extern "C" int rtx_debug_light_plot(rtx_ctx * c, const rtx_point_light * pl, const rtx_spot_light * sl, const rtx_directional_light * dl,
                                    const float * in10, float * out9, int32_t n_light, const float * rgb, uint32_t * packed, int32_t n_plot) {
    if (!c || !pl || !sl || !dl || n_light < 0 || n_plot < 0 || (n_light && (!in10 || !out9)) || (n_plot && (!rgb || !packed))) return RTX_ERR_INVALID_ARG;
    hipSetDevice(c->cfg.device);
    DevBuf din, dout, drgb, dpk;
    int rc = upload(c, din, in10, (size_t)n_light * 40);      // an empty input still gets a (16-byte) buffer: the kernel is handed valid pointers
    if (!rc) rc = ensure(c, dout, (size_t)n_light * 36);
    if (!rc) rc = upload(c, drgb, rgb, (size_t)n_plot * 12);
    if (!rc) rc = ensure(c, dpk, (size_t)n_plot * 4);
    if (rc) return rc;
    const int n = n_light > n_plot ? n_light : n_plot;
    hipLaunchKernelGGL(k_debug_light_plot, dim3((n + 255) / 256), dim3(256), 0, c->stream, *pl, *sl, *dl, (const float *)din.p, (float *)dout.p, (const float *)drgb.p, (uint32_t *)dpk.p, n_light, n_plot);
    HIP_OK(c, hipStreamSynchronize(c->stream));
    if (n_light) HIP_OK(c, hipMemcpy(out9, dout.p, (size_t)n_light * 36, hipMemcpyDeviceToHost));
    if (n_plot) HIP_OK(c, hipMemcpy(packed, dpk.p, (size_t)n_plot * 4, hipMemcpyDeviceToHost));
    return RTX_OK;
}
