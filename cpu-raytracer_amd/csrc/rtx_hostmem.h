// rtx_hostmem.h — who owns the memory behind the C ABI (host code only; included by rtx_api.hip after <hip/hip_runtime.h>).
//
//   DevBuf      one device allocation; move-only, freed by its destructor
//   StageRing   three pinned staging buffers with their events; stage_copy() is the one stream-ordered host -> device upload
//   grow_keep   a bigger device buffer with the old contents in front and zeros behind
//   bind_tables / replace_table   the scene's view of the BLAS, material, texture and sky tables follows every change of a table
//
// One failure rule: a helper that fails leaves every buffer it was given as it found it, and whatever it allocated on the way is released
// by the owner going out of scope.  The context type C only has to carry `std::string err`; stage_copy also reads `c->stream`.  The
// device the memory lives on must be current when an owner dies (rtx_destroy makes it so before it deletes the context).
// Nothing here needs a GPU to be tested: hostmem_check.cpp runs these helpers over counting stand-ins for the HIP calls.
#pragma once
#include <stddef.h>
#include <string.h>
#include <string>
#include <utility>

#define HIP_OK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return RTX_ERR_HIP; } } while (0)

struct DevBuf {
    void * p = nullptr; size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf & operator=(const DevBuf &) = delete;
    DevBuf(DevBuf && o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf & operator=(DevBuf && o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
};

// at least `bytes` of device memory behind b; a buffer that has to grow loses its contents (and, if the allocation fails, its memory)
template <typename C> static int ensure(C * c, DevBuf & b, size_t bytes) {
    if (bytes <= b.cap && b.p) return RTX_OK;
    b.release();
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) { b.p = nullptr; c->err = std::string("hipMalloc: ") + hipGetErrorString(e); return e == hipErrorOutOfMemory ? RTX_ERR_OOM : RTX_ERR_HIP; }
    b.cap = bytes;
    return RTX_OK;
}

template <typename C> static int upload(C * c, DevBuf & b, const void * src, size_t bytes) {
    int rc = ensure(c, b, bytes);
    if (rc) return rc;
    if (bytes) HIP_OK(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return RTX_OK;
}

// out = a new buffer of new_bytes: the first old_bytes of b, then zeros.  b is not touched; the caller has waited for the work that writes it.
template <typename C> static int grown_copy(C * c, const DevBuf & b, size_t old_bytes, size_t new_bytes, const char * what, DevBuf & out) {
    DevBuf nb;
    if (int rc = ensure(c, nb, new_bytes)) return rc;
    hipError_t e = hipMemset(nb.p, 0, nb.cap);
    if (e == hipSuccess && old_bytes) e = hipMemcpy(nb.p, b.p, old_bytes, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { c->err = std::string(what) + " growth: " + hipGetErrorString(e); return RTX_ERR_HIP; }
    out = std::move(nb);
    return RTX_OK;
}

// b grows to new_bytes and keeps its first old_bytes; on failure the old buffer stays in place
template <typename C> static int grow_keep(C * c, DevBuf & b, size_t old_bytes, size_t new_bytes, const char * what) {
    DevBuf nb;
    if (int rc = grown_copy(c, b, old_bytes, new_bytes, what, nb)) return rc;
    b = std::move(nb);
    return RTX_OK;
}

// ---- the four tables kernels reach through the scene they receive by value: BLAS, materials, textures, sky ----
// Binding rule: what a launch sees of a table is what the context holds when the call is made, whether or not a frame was set since the
// table last moved.  bind_tables is the ONE place that writes the eight fields (pointer and count of each table; no memory: no entries), and
// replace_table the one place a table changes: both end every path through it, so no launch site can copy a scene that names a table the
// context no longer holds.  C carries scene, stream, d_blas / h_blas, d_materials / material_count, d_textures / h_tex, d_sky / sky_size.
template <typename C> static void bind_tables(C * c) {
    auto & s = c->scene;
    s.blas = (decltype(s.blas))c->d_blas.p;                s.blas_count = c->d_blas.p ? (int)c->h_blas.size() : 0;
    s.materials = (decltype(s.materials))c->d_materials.p; s.material_count = c->d_materials.p ? c->material_count : 0;
    s.textures = (decltype(s.textures))c->d_textures.p;    s.texture_count = c->d_textures.p ? (int)c->h_tex.size() : 0;
    s.sky = (decltype(s.sky))c->d_sky.p;                   s.sky_size = c->d_sky.p ? c->sky_size : 0;
}

// table = the `bytes` at src: after a wait for the context's stream (queued work still reads the old contents, and a table that moves is
// freed here), in place where it fits, else built beside the old table and swapped in.  Then accept() — the host state that goes with the
// new table: counts, host copies — and the binding.  On failure accept() does not run: table, host state and binding stay what they were.
template <typename C, typename Accept> static int replace_table(C * c, DevBuf & table, const void * src, size_t bytes, Accept && accept) {
    HIP_OK(c, hipStreamSynchronize(c->stream));
    int rc;
    if (bytes <= table.cap && table.p) rc = upload(c, table, src, bytes);
    else { DevBuf nb; rc = upload(c, nb, src, bytes); if (!rc) table = std::move(nb); }
    if (!rc) accept();
    bind_tables(c);
    return rc;
}

// Three pinned buffers taken in turn: the host fills one and queues its copy without waiting for the GPU; a slot is waited for only when
// it comes round again, two uploads later — long finished in steady state.
struct StageRing {
    struct Slot { void * host = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool pending = false; } slot[3];
    int next = 0;
    StageRing() = default;
    StageRing(const StageRing &) = delete;
    StageRing & operator=(const StageRing &) = delete;
    ~StageRing() { for (Slot & s : slot) { if (s.host) hipHostFree(s.host); if (s.done) hipEventDestroy(s.done); } }
};

// dst[0, bytes) = what fill(host) writes into the next slot, by ONE asynchronous copy on the context's stream: ordered after the work already
// queued there (which still reads the previous contents of dst) and before the next call.  A slot too small is replaced by one of grow_to bytes.
template <typename C, typename Fill> static int stage_copy(C * c, StageRing & ring, void * dst, size_t bytes, size_t grow_to, Fill && fill) {
    StageRing::Slot & st = ring.slot[ring.next]; ring.next = (ring.next + 1) % 3;
    if (st.pending) { HIP_OK(c, hipEventSynchronize(st.done)); st.pending = false; }
    if (bytes > st.cap) {
        if (st.host) hipHostFree(st.host);
        st.host = nullptr; st.cap = 0;
        HIP_OK(c, hipHostMalloc(&st.host, grow_to, hipHostMallocDefault)); st.cap = grow_to;
    }
    if (!st.done) HIP_OK(c, hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    fill(st.host);
    HIP_OK(c, hipMemcpyAsync(dst, st.host, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_OK(c, hipEventRecord(st.done, c->stream)); st.pending = true;
    return RTX_OK;
}
// the same from one source array, in slots of exactly the size needed
template <typename C> static int stage_copy(C * c, StageRing & ring, void * dst, const void * src, size_t bytes) {
    return stage_copy(c, ring, dst, bytes, bytes, [&](void * host) { memcpy(host, src, bytes); });
}
