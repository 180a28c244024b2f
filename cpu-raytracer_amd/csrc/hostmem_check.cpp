// hostmem_check.cpp — the owners of rtx_hostmem.h on the CPU: `make hostmem_check` builds this with -fsanitize=address,undefined and runs it.
// The HIP calls the header makes are stand-ins over malloc that count what is live and can be told to fail the n-th allocation, so every
// failure path of DevBuf / ensure / upload / grow_keep / StageRing / stage_copy is walked for leaks, double frees and lost contents.
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

static int live_dev = 0, live_pinned = 0, live_events = 0, allocs = 0, fail_alloc = -1, copies = 0, fail_copy = -1;
static bool alloc_fails() { return allocs++ == fail_alloc; }
static const char * hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
static hipError_t hipMalloc(void ** p, size_t n) { if (alloc_fails()) { *p = nullptr; return hipErrorOutOfMemory; } *p = malloc(n); live_dev++; return hipSuccess; }
static hipError_t hipFree(void * p) { free(p); live_dev--; return hipSuccess; }
static hipError_t hipHostMalloc(void ** p, size_t n, unsigned) { if (alloc_fails()) { *p = nullptr; return hipErrorOutOfMemory; } *p = malloc(n); live_pinned++; return hipSuccess; }
static hipError_t hipHostFree(void * p) { free(p); live_pinned--; return hipSuccess; }
static hipError_t hipMemcpy(void * d, const void * s, size_t n, int) { if (copies++ == fail_copy) return hipErrorUnknown; memcpy(d, s, n); return hipSuccess; }
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
    printf(failures ? "hostmem_check: %d check(s) FAILED\n" : "hostmem_check: ok\n", failures);
    return failures ? 1 : 0;
}
