"""Device-side texture and sky update (include/rtx.h rtx_alloc_texture / rtx_update_texture / rtx_read_texture / rtx_update_sky; kernels
in csrc/rtx_texmip.h) from torch tensors.  Every comparison is bit for bit (NaN == NaN: which NaN inf + -inf yields differs between x86 and
the GPU); there is no tolerance in this file:
  * the chain read back == rtxh_texture_mips of the same level 0, descriptor and texels, for float texels over many exponents with
    subnormals, sums that overflow, infinities, NaNs and -0.0, over shapes on every side of a tile and a pass, at P = 1, 2 and 5;
  * RGBA8: all 256 byte values per channel, the decoded PNG / TGA fixtures == rtxh_texture_load of the file; misaligned buffers;
  * the samplers on adversarial inputs and whole frames of the `materials` scene see the updated texels as they see uploaded ones;
  * stream order without a wait, with RTX_GRAPH=1 replays around the update; a view rendered into a tensor used as a texture;
  * sparse ids, re-allocs, an upload over an allocated id, never-updated textures; every documented status, in the documented order;
  * the sky: samples after update_sky == a probe uploaded from the host, statuses, stream order."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import texset
import util
from test_gpu_textures import sampler_scene, generated, upload, CLS

pytestmark = pytest.mark.gpu

OK, INVALID, LIMIT, STATE = 0, 1, 4, 5
F32, RGBA8 = 0, 1
f32 = np.float32

# (w, h, mipmapped): one texel, strips, one tile, 2 x 2 tiles, non-square chains, strips of tiles, a second pass from level 5 (256 x 256) and on
# a 64 x 2 level (2048 x 64), sides that are no power of two (clipped tiles, no chain), a chain not asked for
SHAPES = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (2, 2, 1), (4, 4, 1), (32, 32, 1), (64, 64, 1), (64, 32, 1), (32, 64, 1), (128, 2, 1), (2, 128, 1),
          (256, 256, 1), (2048, 64, 1), (33, 31, 1), (3, 5, 1), (300, 200, 1), (64, 64, 0)]
PLANTED = np.array([0x00000001, 0x807fffff, 0x00400000, 0x7f7fffff, 0x7f7ffff0, 0xff7fffff, 0x7f000000, 0x7f800000, 0xff800000,
                    0x7fc00000, 0xffc00001, 0x7f800001, 0x80000000, 0x00000000], np.uint32).view(f32)


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_LEVEL0 = {}


def float_level0(w, h):
    """(h, w, 3) float32, seeded: both signs over 70 binary exponents, and planted — in the first texels and in an 8 x 8 block — subnormals,
    values near FLT_MAX whose sums overflow, +-inf, NaNs and -0.0."""
    if (w, h) not in _LEVEL0:
        rng = np.random.default_rng([w, h])
        n = w * h * 3
        bits = (rng.integers(0, 2, n, dtype=np.uint32) << 31) | (rng.integers(90, 160, n, dtype=np.uint32) << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
        t = bits.view(f32).reshape(h, w, 3).copy()
        k = min(n, 42)
        t.reshape(-1)[:k] = PLANTED[(np.arange(k) * 5) % len(PLANTED)]
        if w >= 8 and h >= 10:
            y, x, c = np.mgrid[0:8, 0:8, 0:3]
            t[2:10, 0:8] = PLANTED[(x + 3 * y + 5 * c + (x // 2) * (y // 2)) % len(PLANTED)]
        _LEVEL0[(w, h)] = t
    return _LEVEL0[(w, h)]


def expected(level0, mipmapped=True):
    """The Texture the host builds from level 0 (rtxh_texture_mips: a chain for powers of two), or its level 0 alone."""
    t = texset.texture_from_level0(np.ascontiguousarray(level0, f32))
    return t if mipmapped else texset.unmipped(t)


def assert_texture(got, want, what):
    assert got.desc.tobytes() == want.desc.tobytes(), (what, got.desc, want.desc)
    assert got.texels.shape == want.texels.shape, (what, got.texels.shape, want.texels.shape)
    bad = ~((got.texels.view(np.uint32) == want.texels.view(np.uint32)) | (np.isnan(got.texels) & np.isnan(want.texels))).all(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(bad)} texels differ, first at {np.flatnonzero(bad)[:6].tolist()}"


def level0_of(tex):
    w, h = int(tex.desc["width"][0]), int(tex.desc["height"][0])
    return np.ascontiguousarray(tex.texels[:w * h].reshape(h, w, 3))


def same_frame(a, b, what):
    assert util.bit_exact(a["rgb"], b["rgb"]), f"{what}: {int((a['rgb'].view(np.uint32) != b['rgb'].view(np.uint32)).any(axis=-1).sum())} pixels differ"
    assert np.array_equal(a["packed"], b["packed"]), what


# ---- 1. the chain, f32 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 5])
def test_chain_from_float_texels_equals_the_host_chain(api, monkeypatch, P):
    monkeypatch.setenv("RTX_TEX_PASS_LEVELS", str(P))
    r = api.Renderer(sampler_scene([], 2, 1, 8.0))
    for tid, (w, h, mip) in enumerate(SHAPES):
        level0 = float_level0(w, h)
        r.alloc_texture(tid, w, h, bool(mip))
        r.update_texture(tid, dev(level0))
        assert_texture(r.read_texture(tid), expected(level0, mip), f"P {P}, {w}x{h} mipmapped {mip}")
    for tid, (w, h, mip) in enumerate(SHAPES):                                  # all still there after the later allocs and updates
        assert_texture(r.read_texture(tid), expected(float_level0(w, h), mip), f"P {P}, {w}x{h} again")


def test_chain_of_three_passes_and_buffers_at_odd_addresses(api, monkeypatch):
    import torch
    monkeypatch.setenv("RTX_TEX_PASS_LEVELS", "5")
    r = api.Renderer(sampler_scene([], 2, 1, 8.0))
    level0 = float_level0(2048, 2048)
    r.alloc_texture(0, 2048, 2048, True)
    r.update_texture(0, dev(level0))
    want = expected(level0)
    assert int(want.desc["mip_levels"][0]) == 12
    assert_texture(r.read_texture(0), want, "2048x2048")
    # a float buffer 4 bytes and a byte buffer 1 byte past an allocation's start: aligned to the element, not to the vector
    small = float_level0(64, 32)
    base = torch.empty(64 * 32 * 3 + 1, dtype=torch.float32, device="cuda")
    t = base[1:].view(32, 64, 3); t.copy_(dev(small))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    r.alloc_texture(1, 64, 32, True); r.update_texture(1, t)
    assert_texture(r.read_texture(1), expected(small), "float buffer at + 4 bytes")
    from pyrtx import host
    img = np.random.default_rng(5).integers(0, 256, (32, 64, 4), dtype=np.uint8)
    base8 = torch.empty(64 * 32 * 4 + 1, dtype=torch.uint8, device="cuda")
    t8 = base8[1:].view(32, 64, 4); t8.copy_(dev(img))
    assert t8.is_contiguous() and t8.data_ptr() % 2 == 1
    r.alloc_texture(2, 64, 32, True); r.update_texture(2, t8)
    assert_texture(r.read_texture(2), expected(host.srgb8_to_linear(img[..., :3])), "byte buffer at + 1 byte")


def test_the_default_is_five_levels_per_launch(api, monkeypatch):
    """RTX_TEX_PASS_LEVELS unset: rtxt::DEFAULT_PASS_LEVELS = 5, the measured-faster setting — 2 launches for the 9 levels of
    256 x 256; 8 at P = 1."""
    for P, launches in ((None, 2), (1, 8)):
        if P is None:
            monkeypatch.delenv("RTX_TEX_PASS_LEVELS", raising=False)
        else:
            monkeypatch.setenv("RTX_TEX_PASS_LEVELS", str(P))
        r = api.Renderer(sampler_scene([], 2, 1, 8.0))
        r.alloc_texture(0, 256, 256, True)
        d = dev(float_level0(256, 256))
        r.enable_timing(True)
        r.update_texture(0, d)
        r.synchronize()
        names = [n for n, _ in r.kernel_times()]
        assert len(names) == launches and names[0] == "k_texmip_rgb_f32" and set(names[1:]) == {"k_texmip_chain"}, (P, names)
        r.enable_timing(False)
        assert_texture(r.read_texture(0), expected(float_level0(256, 256)), f"P {P}")


# ---- 2. the chain, RGBA8 -----------------------------------------------------------------------------------------------------------------
IMAGE_FILES = ["images/floor.png", "images/heat_palette.png", "images/png_c6_d8_plain.png", "images/tga_t2_b32.tga", "meshes/LEGOSHLD.tga", "meshes/Floor.png"]


@pytest.mark.parametrize("P", [1, 5])
def test_chain_from_srgb_bytes_equals_the_host_decode(api, monkeypatch, P):
    from pyrtx import host
    monkeypatch.setenv("RTX_TEX_PASS_LEVELS", str(P))
    r = api.Renderer(sampler_scene([], 2, 1, 8.0))
    rng = np.random.default_rng(11)
    img = np.zeros((16, 16, 4), np.uint8)
    for c in range(3):
        img[..., c] = rng.permutation(256).reshape(16, 16)                       # all 256 byte values in each channel
    img[..., 3] = rng.integers(0, 256, (16, 16))
    r.alloc_texture(0, 16, 16, True)
    r.update_texture(0, dev(img))
    assert_texture(r.read_texture(0), expected(host.srgb8_to_linear(img[..., :3])), "all byte values")
    for tid, name in enumerate(IMAGE_FILES, 1):
        path = os.path.join(util.GOLDEN, name)
        px = host.load_image(path)
        assert px.dtype == np.uint8 and px.shape[2] == 4
        h, w = px.shape[:2]
        r.alloc_texture(tid, w, h, True)
        r.update_texture(tid, dev(px))
        got = r.read_texture(tid)
        assert_texture(got, expected(host.srgb8_to_linear(px[..., :3])), name)
        assert_texture(got, host.load_texture(path, True), name + " (rtxh_texture_load)")


# ---- 3. the samplers see it --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["aniso8", "ewa8"])
@pytest.mark.parametrize("name", ["64x16", "300x200"])
def test_samplers_read_the_updated_texels(api, name, config):
    import orc
    mode, mip, aniso = texset.CONFIGS[config]
    tex, in6, lab = generated(name)
    w, h = map(int, name.split("x"))
    r = api.Renderer(sampler_scene([], mode, mip, aniso))
    r.alloc_texture(0, w, h)                                                     # mipmapped: the scene's texture_mode
    r.update_texture(0, dev(level0_of(tex)))
    assert_texture(r.read_texture(0), tex, name)
    util.check_colours(r.debug_texture_sample(0, in6), orc.texture_sample(tex, in6, mode, mip, aniso)[0], lab, CLS, f"{config} {name}")


# ---- 4. whole frames ---------------------------------------------------------------------------------------------------------------------
def allocate_and_update_all(r, sc):
    for tid, t in enumerate(sc.textures):
        r.alloc_texture(tid, int(t.desc["width"][0]), int(t.desc["height"][0]))
        r.update_texture(tid, dev(level0_of(t)))


def test_frames_from_updated_textures_equal_uploaded_ones_and_the_golden(api):
    sc, g = util.load_golden("materials_aniso")
    assert len(sc.textures) >= 1
    host_r = api.Renderer(sc)
    r = api.Renderer(sc)
    allocate_and_update_all(r, sc)
    for tid, t in enumerate(sc.textures):
        assert_texture(r.read_texture(tid), t, f"texture {tid}")
        assert_texture(host_r.read_texture(tid), t, f"uploaded texture {tid}")    # rtx_read_texture of an uploaded id
    for kw in ({}, {"serial": True}):
        out = r.render(**kw)
        same_frame(out, host_r.render(**kw), f"updated vs uploaded {kw}")
        cmp = util.compare_to_golden(out, g)
        assert cmp["stats_equal"] and cmp["nan_mismatch"] == 0 and cmp["packed_mismatch"] == 0 and cmp["max_abs"] == 0.0 and cmp["n_diff_pixels"] == 0, cmp


# ---- 5. stream order without a wait ------------------------------------------------------------------------------------------------------
def two_looks(sc):
    """The level 0 of texture 0 as the scene has it, and a visibly different one of the same shape."""
    a = level0_of(sc.textures[0])
    b = np.ascontiguousarray(a[::-1, ::-1, ::-1]) * f32(0.5) + f32(0.125)
    return a, b


def with_texture0(sc, level0):
    out = copy.copy(sc)
    out.textures = [expected(level0)] + list(sc.textures[1:])
    return out


def test_work_queued_before_the_update_keeps_its_texels(api):
    import torch
    sc, _ = util.load_golden("materials_aniso")
    a, b = two_looks(sc)
    cams = np.concatenate([sc.camera, sc.camera])
    refs = []
    for look in (a, b):
        hr = api.Renderer(with_texture0(sc, look)); hr.set_views(cams)
        refs.append(hr.render_views(0, 1))
    assert not np.array_equal(refs[0]["packed"], refs[1]["packed"])
    r = api.Renderer(sc)
    allocate_and_update_all(r, sc)
    r.set_views(cams)
    H, W = sc.height, sc.width
    da, db = dev(a), dev(b)
    rgb = torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda"); packed = torch.zeros((2, H, W), dtype=torch.int32, device="cuda")
    for _ in range(2):                          # the second round rewrites the texels while the first round's frames may still be running
        r.update_texture(0, db); r.update_texture(0, da)                         # two updates back to back: the last wins
        r.render_views_into(rgb, packed, 0, 1)
        r.update_texture(0, db)
        r.render_views_into(rgb, packed, 1, 1)
    torch.cuda.synchronize()
    got_rgb, got_packed = rgb.cpu().numpy(), packed.cpu().numpy().view(np.uint32)
    for v in range(2):
        assert util.bit_exact(got_rgb[v], refs[v]["rgb"][0]) and np.array_equal(got_packed[v], refs[v]["packed"][0]), f"view {v}"


def test_graph_replay_reads_the_updated_texels(api, monkeypatch):
    """RTX_GRAPH=1: no pointer changes after the alloc, so the captured launches stay valid and read what the update wrote before them."""
    monkeypatch.setenv("RTX_GRAPH", "1")
    sc, _ = util.load_golden("materials_aniso")
    a, b = two_looks(sc)
    refs = [api.Renderer(with_texture0(sc, look)).render(serial=True) for look in (a, b)]
    r = api.Renderer(sc)
    allocate_and_update_all(r, sc)
    da, db = dev(a), dev(b)
    for rounds in range(3):                     # eager, capture, replay
        for d, ref in ((da, refs[0]), (db, refs[1])):
            r.update_texture(0, d)
            same_frame(r.render(serial=True), ref, f"round {rounds}")


# ---- 6. render to texture ----------------------------------------------------------------------------------------------------------------
def test_a_view_rendered_into_a_tensor_becomes_a_texture(api):
    import torch
    from test_gpu_views import camera_set
    sc, _ = util.load_golden("materials_aniso")
    sc.config["width"] = 64; sc.config["height"] = 64
    cams = camera_set(sc)[:2]
    r = api.Renderer(sc)
    allocate_and_update_all(r, sc)
    r.alloc_texture(0, 64, 64)                                                   # the screen: texture 0, whatever shape the scene's own has
    r.set_views(cams)
    rgb = torch.zeros((2, 64, 64, 3), dtype=torch.float32, device="cuda"); packed = torch.zeros((2, 64, 64), dtype=torch.int32, device="cuda")
    r.render_views_into(rgb, packed, 0, 1)
    r.update_texture(0, rgb[0])                                                  # same stream, no wait
    r.render_views_into(rgb, packed, 1, 1)
    torch.cuda.synchronize()
    first = rgb[0].cpu().numpy()
    # the host path: the first frame read back, filtered on the CPU, uploaded
    hr = api.Renderer(sc); hr.set_views(cams)
    black = api.Renderer(with_texture0(sc, np.zeros((64, 64, 3), f32))); black.set_views(cams)
    assert util.bit_exact(first, black.render_views(0, 1)["rgb"][0])             # the screen was black when the first view was rendered
    assert upload(hr, 0, expected(first)) == OK
    want = hr.render_views(1, 1)
    assert util.bit_exact(rgb[1].cpu().numpy(), want["rgb"][0]) and np.array_equal(packed[1].cpu().numpy().view(np.uint32), want["packed"][0])
    assert not np.array_equal(want["packed"][0], black.render_views(1, 1)["packed"][0])      # and the screen is in the second view


# ---- 7. ids and lifetimes ----------------------------------------------------------------------------------------------------------------
def test_sparse_ids_reallocs_and_an_upload_over_an_allocated_id(api):
    r = api.Renderer(sampler_scene([], 2, 1, 8.0))
    lib = r.lib
    rounds = [{0: (64, 32), 5: (33, 31), 40: (2, 2)}, {0: (3, 5), 5: (256, 256), 40: (64, 64)}]
    for ids in rounds:                                                            # the second round: another shape under the same id
        for tid, (w, h) in ids.items():
            r.alloc_texture(tid, w, h, True)
            zero = r.read_texture(tid)
            assert zero.desc.tobytes() == expected(float_level0(w, h)).desc.tobytes() and not zero.texels.view(np.uint32).any(), tid
        for tid, (w, h) in ids.items():
            r.update_texture(tid, dev(float_level0(w, h)))
        for tid, (w, h) in ids.items():
            assert_texture(r.read_texture(tid), expected(float_level0(w, h)), f"id {tid} {w}x{h}")
    for tid in (1, 4, 39, 41):
        assert lib.rtx_read_texture(r.ctx, tid, None, None, 0) == STATE, tid
    # rtx_upload_texture over an allocated id: the chain is the caller's again
    tex = generated("48x48_chain")[0]
    assert upload(r, 5, tex) == OK
    d = dev(float_level0(48, 48))
    assert lib.rtx_update_texture(r.ctx, 5, d.data_ptr(), F32) == STATE
    with pytest.raises(api.RtxError):
        r.update_texture(5, d)                                                    # the right size for what the id holds now: the library's status
    with pytest.raises(ValueError):
        r.update_texture(5, dev(float_level0(256, 256)))                          # the size the id was allocated with before the upload
    assert_texture(r.read_texture(5), tex, "uploaded over an allocated id")
    assert_texture(r.read_texture(0), expected(float_level0(3, 5)), "its neighbour")
    r.alloc_texture(5, 48, 48, True)                                              # and an alloc over the upload
    r.update_texture(5, d)
    assert_texture(r.read_texture(5), expected(float_level0(48, 48)), "allocated over an uploaded id")


def test_a_texture_that_was_never_updated_is_black_and_renders(api):
    sc, _ = util.load_golden("materials_aniso")
    r = api.Renderer(sc)
    black = copy.copy(sc); black.textures = []
    for tid, t in enumerate(sc.textures):
        w, h = int(t.desc["width"][0]), int(t.desc["height"][0])
        r.alloc_texture(tid, w, h)
        black.textures.append(expected(np.zeros((h, w, 3), f32)))
        assert_texture(r.read_texture(tid), black.textures[-1], f"texture {tid}")
    same_frame(r.render(), api.Renderer(black).render(), "never updated")


# ---- 8. statuses -------------------------------------------------------------------------------------------------------------------------
def test_statuses_in_the_documented_order(api):
    from pyrtx.ctypes_structs import RtxTextureDesc
    r = api.Renderer(sampler_scene([generated("64x16")[0]], 2, 1, 8.0))           # id 0: uploaded from the host
    lib = r.lib
    level0 = float_level0(64, 32)
    r.alloc_texture(3, 64, 32, True)
    d = dev(level0)
    r.update_texture(3, d)
    want3, want0 = expected(level0), generated("64x16")[0]

    def unchanged(what):
        assert_texture(r.read_texture(3), want3, what)
        assert_texture(r.read_texture(0), want0, what)
        assert lib.rtx_read_texture(r.ctx, 7, None, None, 0) == STATE, what

    # rtx_alloc_texture: 1. arguments  2. limits
    assert lib.rtx_alloc_texture(None, 3, 8, 8, 1) == INVALID
    for tid, w, h in ((-1, 8, 8), (4096, 8, 8), (3, 0, 8), (3, 8, 0), (3, -4, 8), (-1, 65536, 65536), (3, 0, 1 << 30)):
        assert lib.rtx_alloc_texture(r.ctx, tid, w, h, 1) == INVALID, (tid, w, h)
    assert lib.rtx_alloc_texture(r.ctx, 3, 65536, 65536, 1) == LIMIT              # 17 levels
    assert lib.rtx_alloc_texture(r.ctx, 7, 65536, 32768, 0) == LIMIT              # 2^31 texels
    assert lib.rtx_alloc_texture(r.ctx, 7, 46341, 46341, 1) == LIMIT
    unchanged("after refused allocs")
    # rtx_update_texture: 1. pointer and format  2. state
    assert lib.rtx_update_texture(None, 3, d.data_ptr(), F32) == INVALID
    for tid in (3, 7, -1):                                                        # the pointer and the format come before the id
        assert lib.rtx_update_texture(r.ctx, tid, None, F32) == INVALID
        assert lib.rtx_update_texture(r.ctx, tid, d.data_ptr() + 2, F32) == INVALID
        assert lib.rtx_update_texture(r.ctx, tid, d.data_ptr() + 1, F32) == INVALID
        assert lib.rtx_update_texture(r.ctx, tid, d.data_ptr(), 2) == INVALID
        assert lib.rtx_update_texture(r.ctx, tid, d.data_ptr(), -1) == INVALID
    for tid in (7, -1, 4096, 2, 0):                                               # never created; 0: uploaded, not allocated
        assert lib.rtx_update_texture(r.ctx, tid, d.data_ptr(), F32) == STATE, tid
        assert lib.rtx_update_texture(r.ctx, tid, d.data_ptr() + 1, RGBA8) == STATE, tid
    unchanged("after refused updates")
    # rtx_read_texture
    desc = RtxTextureDesc()
    n = len(want3.texels)
    buf = np.full((n, 3), -1.0, f32)
    assert lib.rtx_read_texture(None, 3, None, None, 0) == INVALID
    assert lib.rtx_read_texture(r.ctx, -1, None, None, 0) == INVALID and lib.rtx_read_texture(r.ctx, 4096, None, None, 0) == INVALID
    assert lib.rtx_read_texture(r.ctx, 3, C.byref(desc), buf.ctypes.data, n - 1) == INVALID and bool((buf == -1.0).all())
    assert lib.rtx_read_texture(r.ctx, 3, None, buf.ctypes.data, 0) == INVALID
    assert lib.rtx_read_texture(r.ctx, 7, C.byref(desc), buf.ctypes.data, n) == STATE and bool((buf == -1.0).all())
    assert lib.rtx_read_texture(r.ctx, 3, C.byref(desc), None, 0) == OK and (desc.width, desc.height, desc.mip_levels) == (64, 32, 6)
    assert lib.rtx_read_texture(r.ctx, 3, None, None, 0) == OK
    assert lib.rtx_read_texture(r.ctx, 3, None, buf.ctypes.data, n) == OK and util.bit_exact(buf, want3.texels)
    # the Python checks reach nothing either
    for bad in (d.cpu(), d.double(), d[:, :32], d[:16], dev(np.zeros((32, 64, 3), np.uint8))):
        with pytest.raises(ValueError):
            r.update_texture(3, bad)
    unchanged("after refused Python calls")
    r.update_texture(3, dev(level0[::-1]))                                        # and the context still works
    assert_texture(r.read_texture(3), expected(level0[::-1]), "after everything")


# ---- 9. the sky --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 2, 64])
def test_sky_updated_from_a_tensor_equals_an_uploaded_probe(api, size):
    import orc
    old = texset.sky_probe(size, seed=9)
    new = util.load_golden("cube")[0].sky if size == 64 else texset.sky_probe(size)
    assert new.shape == (size, size, 3) and not np.array_equal(old, new)
    dirs, _ = texset.sky_directions(size, 256)
    r = api.Renderer(sampler_scene([], 2, 1, 8.0, old))
    host_r = api.Renderer(sampler_scene([], 2, 1, 8.0, new))
    util.check_colours(r.debug_sky_sample(dirs), orc.sky_sample(old, dirs), what=f"sky {size} before")
    r.update_sky(dev(new))
    got = r.debug_sky_sample(dirs)
    util.check_colours(got, host_r.debug_sky_sample(dirs), what=f"sky {size} vs uploaded")
    util.check_colours(got, orc.sky_sample(new, dirs), what=f"sky {size} vs oracle")      # the clamp's padding texel included: still zero


def test_sky_statuses_and_stream_order(api):
    import torch
    sc, _ = util.load_golden("cube")
    size = sc.sky.shape[0]
    new = np.ascontiguousarray(sc.sky[::-1, ::-1, ::-1]) * f32(0.5)
    d = dev(new)
    r0 = api.Renderer(sc, upload=False)
    assert r0.lib.rtx_update_sky(r0.ctx, d.data_ptr(), 1) == STATE and r0.lib.rtx_update_sky(r0.ctx, d.data_ptr(), size) == STATE      # before rtx_upload_sky
    assert r0.lib.rtx_update_sky(r0.ctx, None, size) == INVALID
    r0.close()
    cams = np.concatenate([sc.camera, sc.camera])
    refs = []
    for sky in (sc.sky, new):
        s2 = copy.copy(sc); s2.sky = sky
        hr = api.Renderer(s2); hr.set_views(cams)
        refs.append(hr.render_views(0, 1))
    assert not np.array_equal(refs[0]["packed"], refs[1]["packed"])
    r = api.Renderer(sc)
    lib = r.lib
    assert lib.rtx_update_sky(None, d.data_ptr(), size) == INVALID
    assert lib.rtx_update_sky(r.ctx, None, size) == INVALID and lib.rtx_update_sky(r.ctx, d.data_ptr() + 2, size) == INVALID
    for s in (size - 1, size + 1, 0, -1, 2 * size):
        assert lib.rtx_update_sky(r.ctx, d.data_ptr(), s) == INVALID, s
    with pytest.raises(api.RtxError):
        r.update_sky(dev(np.zeros((size // 2, size // 2, 3), f32)))
    r.set_views(cams)
    H, W = sc.height, sc.width
    rgb = torch.zeros((2, H, W, 3), dtype=torch.float32, device="cuda"); packed = torch.zeros((2, H, W), dtype=torch.int32, device="cuda")
    r.render_views_into(rgb, packed, 0, 1)                                       # queued before the update: the old sky
    r.update_sky(d)
    r.render_views_into(rgb, packed, 1, 1)
    torch.cuda.synchronize()
    for v in range(2):
        assert util.bit_exact(rgb[v].cpu().numpy(), refs[v]["rgb"][0]) and np.array_equal(packed[v].cpu().numpy().view(np.uint32), refs[v]["packed"][0]), f"view {v}"
