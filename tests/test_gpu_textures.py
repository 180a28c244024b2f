"""Sample-level parity of the texture and sky samplers (csrc/rtx_texture.h through rtx_debug_texture_sample / rtx_debug_sky_sample; one
Renderer per sampler configuration: mode and filter are read in rtx_create) on adversarial inputs (tests/texset.py: texel centres and
corners, negative and huge coordinates, +-0 / inf / NaN, zero derivatives, LODs on level boundaries, every anisotropic tap count,
eccentric and tiny EWA footprints) over synthetic textures no file of the goldens has: 1x1, 2x2, strips, non-square chains, sides that
are no power of two, a caller-made chain on a 48x48 base, float texels with inf and subnormals.  Every comparison is bit for bit
(NaN == NaN); there is no tolerance in this file:
  * against the REAL reference's colours (tests/golden/unit/texprobe_<build>.npz, see test_texture_probes.py);
  * against the batch oracle on generated sets over every texture and nine sampler configurations;
  * at batch sizes around a wave and a block and one of 1e5 samples;
  * after uploads at sparse ids and re-uploads of another shape under the same id;
  * whole frames of the `materials` scene with its textures replaced by 300x200, 64x16 and 256x1, every launch shape, incl. the
    instrumented kernels' texel-fetch counter;
  * the sky on axes, poles, |z| > 1, degenerate directions and the inclusive index clamp, for probes of size 1, 2 and 64."""
import copy
import ctypes as C

import numpy as np
import pytest

import texset
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def sampler_scene(textures, mode, mip, aniso, sky=None):
    """The cube golden scene (nothing of it is rendered here) carrying `textures` and the sampler configuration."""
    sc = copy.deepcopy(util.load_golden("cube")[0])
    sc.config["texture_mode"] = mode; sc.config["mip_filter"] = mip; sc.config["max_anisotropy"] = aniso
    sc.textures = list(textures)
    if sky is not None:
        sc.sky = sky
    return sc


_SETS = {}


def generated(name, n=160, seed=7):
    """(texture, in6, label indices) of one texset texture, cached per module run: >= 2048 samples, every class."""
    if (name, n, seed) not in _SETS:
        tex = texset.float_texture(name) if name in texset.FLOAT_TEXTURES else texset.texture8(*map(int, name.split("x")))
        in6, labels = texset.generate(tex, n, seed)
        assert len(in6) >= 2048
        _SETS[(name, n, seed)] = (tex, in6, texset.label_index(labels))
    return _SETS[(name, n, seed)]


ALL_NAMES = [texset.name8(w, h) for w, h in texset.SHAPES8] + texset.FLOAT_TEXTURES
CLS = np.array(texset.CLASSES)


# ---- the reference's own colours -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", list(util.TEX_PROBES))
def test_samplers_reproduce_reference_texture_probes(api, build):
    import orc
    P = util.load_tex_probe(build)
    mode, mip, aniso = util.TEX_PROBES[build]
    texs = [texset.texture8(w, h, P["tile_" + texset.name8(w, h)]) for w, h in texset.SHAPES8]
    if mode != 2:
        texs = [texset.unmipped(t) for t in texs]                              # such builds of the reference hold no chain
    r = api.Renderer(sampler_scene(texs, mode, mip, aniso))
    for k, name in enumerate(P["names"]):
        in6 = P["in_" + name]
        assert orc.texture_sample(texs[k], in6, mode, mip, aniso)[1].max() <= texset.MAX_FETCHES
        util.check_colours(r.debug_texture_sample(k, in6), P["ref_" + name], P["label_" + name], P["classes"], f"{build} {name}")


# ---- generated sets against the batch oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(texset.CONFIGS))
def test_generated_samples_equal_the_oracle(api, config):
    """Every synthetic texture x this sampler configuration, small textures first."""
    import orc
    mode, mip, aniso = texset.CONFIGS[config]
    order = sorted(ALL_NAMES, key=lambda n: len(generated(n)[0].texels))
    r = api.Renderer(sampler_scene([generated(n)[0] for n in order], mode, mip, aniso))
    for k, name in enumerate(order):
        tex, in6, lab = generated(name)
        want, fetches = orc.texture_sample(tex, in6, mode, mip, aniso)
        assert fetches.max() <= texset.MAX_FETCHES
        util.check_colours(r.debug_texture_sample(k, in6), want, lab, CLS, f"{config} {name}")


# ---- batch sizes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 100_003])
def test_batch_sizes_around_a_wave_and_a_block(api, n):
    """Partial waves and blocks of the debug kernel, one sample past each, and a batch of many blocks: each result in its own slot."""
    import orc
    mode, mip, aniso = texset.CONFIGS["ewa8"]
    tex, in6, lab = generated("64x16")
    rng = np.random.default_rng(n)
    pick = rng.permutation(len(in6))[:n] if n <= len(in6) else rng.integers(len(in6), size=n)
    x = in6[pick].copy()
    if n > len(in6):
        x[:, 0] = rng.uniform(-2, 2, n).astype(np.float32)                      # every sample distinct in s
    want, fetches = orc.texture_sample(tex, x, mode, mip, aniso, threads=16)
    assert fetches.max() <= texset.MAX_FETCHES
    r = api.Renderer(sampler_scene([tex], mode, mip, aniso))
    util.check_colours(r.debug_texture_sample(0, x), want, lab[pick], CLS, f"batch of {n}")


# ---- upload paths ----------------------------------------------------------------------------------------------------------------------
def upload(r, tid, tex):
    from pyrtx.ctypes_structs import RtxTextureDesc
    desc = RtxTextureDesc()
    C.memmove(C.byref(desc), tex.desc.ctypes.data, C.sizeof(RtxTextureDesc))
    t = np.ascontiguousarray(tex.texels, np.float32)
    return r.lib.rtx_upload_texture(r.ctx, tid, C.byref(desc), t.ctypes.data, len(t))


def test_sparse_ids_and_reupload_under_the_same_id(api):
    """Textures at ids 0, 5 and 40 (the ids between were never uploaded), then another shape under each id (rtx_upload_texture releases the
    old texel array), then the first shapes again: every sample the oracle's for the texture that id holds at that moment."""
    import orc
    mode, mip, aniso = texset.CONFIGS["aniso8"]
    r = api.Renderer(sampler_scene([generated("32x32")[0]], mode, mip, aniso))
    rounds = [{0: "64x16", 5: "300x200", 40: "2x2"}, {0: "3x5", 5: "16x64", 40: "48x48_chain"}, {0: "64x16", 5: "1x1", 40: "1024x1024"}]
    for ids in rounds:
        for tid, name in ids.items():
            assert upload(r, tid, generated(name)[0]) == 0
        for tid, name in ids.items():
            tex, in6, lab = generated(name)
            util.check_colours(r.debug_texture_sample(tid, in6), orc.texture_sample(tex, in6, mode, mip, aniso)[0], lab, CLS, f"id {tid} {name}")
    one = np.zeros((1, 6), np.float32); out = np.zeros((1, 3), np.float32)
    for tid in (1, 39, 41, -1, 4096):                                           # never uploaded / out of range: a status, not a launch
        assert r.lib.rtx_debug_texture_sample(r.ctx, tid, one.ctypes.data, out.ctypes.data, 1) == 1, tid


def test_chains_the_samplers_cannot_index_are_refused(api):
    """A level whose extent would be zero (one level more than min(w, h) allows), an offset before the array or a level reaching past it:
    RTX_ERR_INVALID_ARG, and the id keeps what it held."""
    import orc
    mode, mip, aniso = texset.CONFIGS["trilinear"]
    tex, in6, lab = generated("64x16")
    r = api.Renderer(sampler_scene([tex], mode, mip, aniso))
    for mutate in ("extra_level", "negative_offset", "offset_past_end", "no_levels", "zero_width"):
        bad = copy.deepcopy(tex)
        if mutate == "extra_level":
            bad.desc["mip_levels"] = 6; bad.desc["mip_offsets"][0, 5] = 0
        elif mutate == "negative_offset":
            bad.desc["mip_offsets"][0, 2] = -1
        elif mutate == "offset_past_end":
            bad.desc["mip_offsets"][0, 4] = len(tex.texels) - 3                 # the 4x1 level would end one texel past the array
        elif mutate == "no_levels":
            bad.desc["mip_levels"] = 0
        else:
            bad.desc["width"] = 0
        assert upload(r, 0, bad) == 1, mutate
    util.check_colours(r.debug_texture_sample(0, in6), orc.texture_sample(tex, in6, mode, mip, aniso)[0], lab, CLS, "after refusals")


# ---- whole frames ----------------------------------------------------------------------------------------------------------------------
FRAME_CONFIGS = ["materials_aniso", "materials_trilinear", "materials_ewa", "materials_bilinear", "materials_aniso2"]
FRAME_TEXTURES = [("300x200", "64x16"), ("64x16", "256x1"), ("256x1", "300x200")]


def frame_scene(golden, names):
    sc, _ = util.load_golden(golden)
    assert len(sc.textures) == 2
    texs = [generated(n)[0] for n in names]
    sc.textures = [t if int(sc.config["texture_mode"][0]) == 2 else texset.unmipped(t) for t in texs]
    return sc


@pytest.mark.parametrize("names", FRAME_TEXTURES, ids="_".join)
@pytest.mark.parametrize("golden", FRAME_CONFIGS)
def test_frames_with_odd_textures_equal_the_oracle(api, golden, names):
    """The materials scene (textured plane and mesh, dielectric spheres, three bounces) with a texture without mips, a non-square chain and
    a one-level strip in place of its two square ones: rgb bits, packed pixels and ray counts in every launch shape."""
    import orc
    from test_gpu_parity import MODES
    sc = frame_scene(golden, names)
    ref = orc.OracleScene(sc).render(threads=16)
    r = api.Renderer(sc)
    for mode, kw in MODES.items():
        out = r.render(**kw)
        assert out["stats"] == ref["stats"], (mode, out["stats"], ref["stats"])
        assert util.bit_exact(out["rgb"], ref["rgb"]), (mode, int((out["rgb"].view(np.uint32) != ref["rgb"].view(np.uint32)).any(axis=-1).sum()))
        assert np.array_equal(out["packed"], ref["packed"]), mode


@pytest.mark.parametrize("golden", FRAME_CONFIGS)
def test_texel_fetch_counter_through_the_odd_textures(api, golden):
    """The instrumented kernels' texel_fetches (the modulo wrap, the paired anisotropic taps, EWA's rows) == the oracle's count."""
    import orc
    sc = frame_scene(golden, FRAME_TEXTURES[0])
    ref = orc.OracleScene(sc).render(threads=16)
    out = api.Renderer(sc).render(count_work=True)
    assert out["work"]["texel_fetches"] == ref["work"]["texel_fetches"] and ref["work"]["texel_fetches"] > 0
    assert out["stats"] == ref["stats"] and util.bit_exact(out["rgb"], ref["rgb"]) and np.array_equal(out["packed"], ref["packed"])


# ---- sky -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 2, 64])
def test_sky_sample_on_poles_clamps_and_degenerate_directions(api, size):
    import orc
    sky = util.load_golden("cube")[0].sky if size == 64 else texset.sky_probe(size)
    assert sky.shape[0] == size
    dirs, labels = texset.sky_directions(size, 256)
    want = orc.sky_sample(sky, dirs)
    r = api.Renderer(sampler_scene([], 2, 1, 8.0, sky))
    classes = np.array(texset.SKY_CLASSES)
    lab = np.array([texset.SKY_CLASSES.index(x) for x in labels])
    util.check_colours(r.debug_sky_sample(dirs), want, lab, classes, f"sky {size}")
    for n in (1, 63, 65, 257):
        util.check_colours(r.debug_sky_sample(dirs[:n]), want[:n], lab[:n], classes, f"sky {size} batch {n}")
