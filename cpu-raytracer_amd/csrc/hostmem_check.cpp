// hostmem_check.cpp — the owners of rtx_hostmem.h on the CPU: `make hostmem_check` builds this with -fsanitize=address,undefined and runs it.
// The HIP calls the header makes are stand-ins over malloc that count what is live and can be told to fail the n-th allocation, so every
// failure path of DevBuf / ensure / upload / grow_keep / StageRing / stage_copy is walked for leaks, double frees and lost contents.
// The last sections pin the binding rule of the four scene tables (bind_tables / replace_table): each table is grown past its capacity after
// a scene was bound, and the bound pointer and count must be the context's own, the old table freed exactly once and only after a wait
// for the stream, also when the growth's allocation or copy fails.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/rtx.h"

typedef int hipError_t;
typedef struct Ev * hipEvent_t;
typedef void * hipStream_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
enum { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice, hipHostMallocDefault = 0, hipEventDisableTiming = 2 };
struct Ev { int recorded = 0; };

static int live_dev = 0, live_pinned = 0, live_events = 0, allocs = 0, fail_alloc = -1, copies = 0, fail_copy = -1, syncs = 0, unsynced_frees = 0;
static std::vector<void *> freed;          // every device pointer freed, in order; a stream wait clears `dirty`, queued work (the tests say when) sets it
static bool dirty = false;
static bool alloc_fails() { return allocs++ == fail_alloc; }
static const char * hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
static hipError_t hipMalloc(void ** p, size_t n) { if (alloc_fails()) { *p = nullptr; return hipErrorOutOfMemory; } *p = malloc(n); live_dev++; return hipSuccess; }
static hipError_t hipFree(void * p) { free(p); live_dev--; freed.push_back(p); if (dirty) unsynced_frees++; return hipSuccess; }
static hipError_t hipStreamSynchronize(hipStream_t) { syncs++; dirty = false; return hipSuccess; }
static hipError_t hipHostMalloc(void ** p, size_t n, unsigned) { if (alloc_fails()) { *p = nullptr; return hipErrorOutOfMemory; } *p = malloc(n); live_pinned++; return hipSuccess; }
static hipError_t hipHostFree(void * p) { free(p); live_pinned--; return hipSuccess; }
static int unsynced_copies = 0;
static hipError_t hipMemcpy(void * d, const void * s, size_t n, int) { if (dirty) unsynced_copies++; if (copies++ == fail_copy) return hipErrorUnknown; memcpy(d, s, n); return hipSuccess; }
static hipError_t hipMemcpyAsync(void * d, const void * s, size_t n, int k, hipStream_t) { return hipMemcpy(d, s, n, k); }
static hipError_t hipMemset(void * d, int v, size_t n) { memset(d, v, n); return hipSuccess; }
static hipError_t hipEventCreateWithFlags(hipEvent_t * e, unsigned) { *e = new Ev(); live_events++; return hipSuccess; }
static hipError_t hipEventDestroy(hipEvent_t e) { delete e; live_events--; return hipSuccess; }
static hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { e->recorded++; return hipSuccess; }
static hipError_t hipEventSynchronize(hipEvent_t e) { return e->recorded ? hipSuccess : hipErrorUnknown; }

#include "rtx_hostmem.h"

struct Ctx { std::string err; hipStream_t stream = nullptr; };
static int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); failures++; } } while (0)
static bool holds(const DevBuf & b, size_t from, size_t to, unsigned char v) { for (size_t i = from; i < to; i++) if (((unsigned char *)b.p)[i] != v) return false; return true; }

// The table part of a context, with the member names bind_tables reads, and a scene with the eight fields it writes.
struct Scene { const int32_t * blas; int32_t blas_count; const float * materials; int32_t material_count; const int16_t * textures; int32_t texture_count; const float * sky; int32_t sky_size; };
struct TableCtx {
    std::string err; hipStream_t stream = nullptr; Scene scene = {};
    DevBuf d_blas, d_materials, d_textures, d_sky;
    std::vector<int32_t> h_blas; std::vector<int16_t> h_tex; int material_count = 0, sky_size = 0;
};
// the four growth calls as rtx_api.hip makes them: the new table staged beside the host state, which accept() swaps in
static int put_blas(TableCtx * t, size_t id, int32_t v) {
    std::vector<int32_t> table = t->h_blas; if (id >= table.size()) table.resize(id + 1, 0); table[id] = v;
    return replace_table(t, t->d_blas, table.data(), table.size() * 4, [&] { t->h_blas.swap(table); });
}
static int put_materials(TableCtx * t, int count, float v) {
    std::vector<float> m((size_t)count, v);
    return replace_table(t, t->d_materials, m.data(), m.size() * 4, [&] { t->material_count = count; });
}
static int put_texture(TableCtx * t, size_t id, int16_t v) {
    std::vector<int16_t> table = t->h_tex; if (id >= table.size()) table.resize(id + 1, 0); table[id] = v;
    return replace_table(t, t->d_textures, table.data(), table.size() * 2, [&] { t->h_tex.swap(table); });
}
static int put_sky(TableCtx * t, int size, float v) {
    std::vector<float> s((size_t)size * size * 3 + 3, v);
    return replace_table(t, t->d_sky, s.data(), s.size() * 4, [&] { t->sky_size = size; });
}
// the scene names exactly what the context holds: all four tables, pointers and counts
static bool bound(const TableCtx & t) {
    const Scene & s = t.scene;
    return (const void *)s.blas == t.d_blas.p && s.blas_count == (t.d_blas.p ? (int)t.h_blas.size() : 0) &&
           (const void *)s.materials == t.d_materials.p && s.material_count == (t.d_materials.p ? t.material_count : 0) &&
           (const void *)s.textures == t.d_textures.p && s.texture_count == (t.d_textures.p ? (int)t.h_tex.size() : 0) &&
           (const void *)s.sky == t.d_sky.p && s.sky_size == (t.d_sky.p ? t.sky_size : 0);
}
static int times_freed(const void * p) { int n = 0; for (void * q : freed) n += q == p; return n; }

// One table after a scene was bound: `grow(k)` makes it hold k entries (k = 1, 2, ... each larger than the last), `count()` is the context's
// count of it.  Growth past the capacity moves the table: bound to the new one, the old one freed once, after the wait.  A growth whose
// allocation or copy fails leaves table, count and binding alone and frees nothing.  A smaller table (materials, sky; an id table never
// shrinks) stays in place and only the count moves.
template <typename Grow, typename Count> static void table_section(TableCtx & t, DevBuf & table, bool shrinks, Grow grow, Count count) {
    CHECK(grow(2) == RTX_OK && bound(t));
    bind_tables(&t);                                                    // "rtx_set_frame"
    for (int k = 3; k <= 40; k += k < 5 ? 1 : 35) {                     // 3, 4, 5, 40: past the exact capacity every time
        void * const old = table.p; const int frees0 = (int)freed.size(), syncs0 = syncs;
        dirty = true;                                                   // a frame is queued that reads the old table
        CHECK(grow(k) == RTX_OK);
        CHECK(table.p && table.p != old);                               // built beside the old one: the address is certain to differ
        CHECK(bound(t) && count() == k);
        CHECK((int)freed.size() == frees0 + 1 && freed.back() == old && times_freed(old) == 1);
        CHECK(syncs > syncs0 && unsynced_frees == 0 && unsynced_copies == 0);
    }
    {   // the allocation of a growth fails: nothing moved, nothing freed, nothing rebound to something else
        void * const old = table.p; const int frees0 = (int)freed.size(), n0 = count(); const Scene s0 = t.scene;
        fail_alloc = allocs; CHECK(grow(200) == RTX_ERR_OOM && !t.err.empty());
        fail_alloc = -1;
        CHECK(table.p == old && count() == n0 && bound(t) && memcmp(&s0, &t.scene, sizeof(Scene)) == 0 && (int)freed.size() == frees0);
    }
    {   // the copy into the new table fails: the new table is released, the old one stays bound
        void * const old = table.p; const int frees0 = (int)freed.size(), n0 = count();
        fail_copy = copies; CHECK(grow(200) == RTX_ERR_HIP);
        fail_copy = -1;
        CHECK(table.p == old && count() == n0 && bound(t) && (int)freed.size() == frees0 + 1 && times_freed(old) == 0);
    }
    {   // fewer entries fit in place: the pointer stays, the count must still follow
        void * const old = table.p; const int frees0 = (int)freed.size(), want = shrinks ? 7 : count();
        dirty = true;
        CHECK(grow(7) == RTX_OK && table.p == old && count() == want && bound(t) && (int)freed.size() == frees0 && unsynced_copies == 0);
        CHECK(grow(200) == RTX_OK && table.p != old && count() == 200 && bound(t) && times_freed(old) == 1);       // and the growth that failed twice succeeds
    }
}

int main() {
    Ctx c;
    {   // ownership: moves hand the allocation over, the destructor of the last owner frees it once
        DevBuf a; CHECK(ensure(&c, a, 100) == RTX_OK && a.cap == 100 && live_dev == 1);
        void * was = a.p;
        CHECK(ensure(&c, a, 50) == RTX_OK && a.p == was);                // large enough: kept
        DevBuf b(std::move(a)); CHECK(!a.p && !a.cap && b.p == was && live_dev == 1);
        DevBuf d; CHECK(ensure(&c, d, 8) == RTX_OK && live_dev == 2);
        d = std::move(b); CHECK(d.p == was && !b.p && live_dev == 1);   // the target's old memory is released
        d = std::move(d); CHECK(d.p == was && live_dev == 1);
        CHECK(ensure(&c, a, 0) == RTX_OK && a.cap == 16);                // an empty request still yields a valid pointer
        std::vector<DevBuf> v; v.push_back(std::move(d)); v.resize(40); v.push_back(std::move(a)); CHECK(live_dev == 2);      // reallocation moves
    }
    CHECK(live_dev == 0);
    {   // ensure / upload under a failing allocation: an error code, no memory held, nothing freed twice
        DevBuf a; unsigned char src[64]; memset(src, 7, sizeof(src));
        CHECK(upload(&c, a, src, 64) == RTX_OK && holds(a, 0, 64, 7));
        fail_alloc = allocs; CHECK(ensure(&c, a, 128) == RTX_ERR_OOM && !a.p && !a.cap && live_dev == 0 && !c.err.empty());
        fail_alloc = -1; fail_copy = copies; CHECK(upload(&c, a, src, 64) == RTX_ERR_HIP && live_dev == 1);
        fail_copy = -1;
    }
    CHECK(live_dev == 0);
    {   // grow_keep: old contents in front, zeros behind; on failure the old buffer stays, untouched
        DevBuf a; unsigned char src[32]; memset(src, 9, sizeof(src));
        CHECK(upload(&c, a, src, 32) == RTX_OK);
        CHECK(grow_keep(&c, a, 32, 96, "test") == RTX_OK && a.cap == 96 && holds(a, 0, 32, 9) && holds(a, 32, 96, 0) && live_dev == 1);
        void * was = a.p;
        fail_alloc = allocs; CHECK(grow_keep(&c, a, 96, 200, "test") == RTX_ERR_OOM && a.p == was && a.cap == 96 && holds(a, 0, 32, 9) && live_dev == 1);
        fail_alloc = -1; fail_copy = copies; CHECK(grow_keep(&c, a, 96, 200, "test") == RTX_ERR_HIP && a.p == was && a.cap == 96 && live_dev == 1);
        fail_copy = -1;
        DevBuf fresh; CHECK(grow_keep(&c, fresh, 0, 10, "test") == RTX_OK && holds(fresh, 0, 10, 0));      // first use: nothing to keep
        DevBuf x, y;                                                    // grown_copy: the pair grows together or not at all
        CHECK(grown_copy(&c, a, 96, 120, "test", x) == RTX_OK && a.p == was && x.cap == 120 && holds(x, 0, 32, 9) && live_dev == 3);
        fail_alloc = allocs; CHECK(grown_copy(&c, fresh, 10, 20, "test", y) == RTX_ERR_OOM && !y.p && fresh.cap == 10);
        fail_alloc = -1;
    }
    CHECK(live_dev == 0);
    {   // the staging ring: five uploads of 1, 3, 2, 5, 4 units wrap the three slots and grow them; a failed pinned allocation leaks nothing
        StageRing ring; DevBuf dst; CHECK(ensure(&c, dst, 5 * 16) == RTX_OK);
        const int units[5] = { 1, 3, 2, 5, 4 };
        for (int k = 0; k < 5; k++) {
            unsigned char src[5 * 16]; memset(src, 10 + k, sizeof(src));
            const size_t bytes = (size_t)units[k] * 16;
            CHECK(stage_copy(&c, ring, dst.p, src, bytes) == RTX_OK && holds(dst, 0, bytes, (unsigned char)(10 + k)));
        }
        CHECK(ring.next == 2 && live_pinned == 3 && live_events == 3 && ring.slot[0].cap == 5 * 16 && ring.slot[1].cap == 4 * 16 && ring.slot[2].cap == 2 * 16);
        // a fill callback and a growth policy of its own (the frame block): pieces at offsets, half as much again
        CHECK(stage_copy(&c, ring, dst.p, 48, 72, [](void * h) { memset(h, 1, 16); memset((char *)h + 16, 2, 32); }) == RTX_OK);
        CHECK(ring.slot[2].cap == 72 && holds(dst, 0, 16, 1) && holds(dst, 16, 48, 2));
        fail_alloc = allocs; unsigned char big[5 * 16] = {};
        StageRing small; CHECK(stage_copy(&c, small, dst.p, big, sizeof(big)) == RTX_ERR_HIP && live_pinned == 3 && !small.slot[0].host && !small.slot[0].cap);
        fail_alloc = -1;
        CHECK(stage_copy(&c, small, dst.p, big, 16) == RTX_OK && live_pinned == 4);       // the ring works on after the failure
    }
    CHECK(live_dev == 0 && live_pinned == 0 && live_events == 0);
    {   // the scene tables: nothing held binds to nothing; then each table in turn grows after the bind, the other three staying bound
        TableCtx t; bind_tables(&t);
        CHECK(bound(t) && !t.scene.blas && !t.scene.blas_count && !t.scene.sky && !t.scene.sky_size);
        freed.clear();
        table_section(t, t.d_blas, false, [&](int k) { return put_blas(&t, (size_t)k - 1, k); }, [&] { return (int)t.h_blas.size(); });
        freed.clear();
        table_section(t, t.d_materials, true, [&](int k) { return put_materials(&t, k, 0.5f); }, [&] { return t.material_count; });
        freed.clear();
        table_section(t, t.d_textures, false, [&](int k) { return put_texture(&t, (size_t)k - 1, (int16_t)k); }, [&] { return (int)t.h_tex.size(); });
        freed.clear();
        table_section(t, t.d_sky, true, [&](int k) { return put_sky(&t, k, 0.25f); }, [&] { return t.sky_size; });
        CHECK(live_dev == 4 && t.h_blas[39] == 40 && ((const int32_t *)t.d_blas.p)[39] == 40 && ((const int32_t *)t.d_blas.p)[2] == 3);      // the table kept what the ids held
        fail_alloc = allocs; CHECK(put_sky(&t, 300, 0.0f) == RTX_ERR_OOM && t.scene.sky == t.d_sky.p && t.scene.sky_size == 200);        // a failed growth names live memory
        fail_alloc = -1;
    }
    CHECK(live_dev == 0);
    printf(failures ? "hostmem_check: %d check(s) FAILED\n" : "hostmem_check: ok\n", failures);
    return failures ? 1 : 0;
}
