"""The oracle's samplers against the REAL reference's texture probes, and the invariants of tests/texset.py (CPU only).
  * the seeded probes of the frame goldens (texprobe0 / texprobe1: Floor.png, LEGOSHLD.tga; five sampler builds) and the adversarial ones
    of tests/golden/unit/texprobe_<build>.npz (six builds, eleven synthetic textures), bit for bit, NaN == NaN;
  * the textures: the host library's chain == an independent numpy chain == what host.load_texture decodes from a PNG of the same pixels;
  * the sample sets: class counts, the cost condition, determinism."""
import os

import numpy as np
import pytest

import orc
import texset
import util
from pyrtx import host


@pytest.mark.parametrize("name", ["materials_aniso", "materials_trilinear", "materials_ewa", "materials_bilinear", "materials_aniso2"])
def test_oracle_reproduces_the_seeded_reference_probes(name):
    sc, g = util.load_golden(name)
    cf = sc.config
    sizes = [(int(t.desc["width"][0]), int(t.desc["height"][0])) for t in sc.textures]
    for k, wh in enumerate([(32, 32), (256, 256)]):
        probe = g[f"texprobe{k}"]
        out, _ = orc.texture_sample(sc.textures[sizes.index(wh)], probe[:, :6], int(cf["texture_mode"][0]), int(cf["mip_filter"][0]), float(cf["max_anisotropy"][0]))
        util.check_colours(out, probe[:, 6:9], what=f"{name} texprobe{k}")


@pytest.mark.parametrize("build", list(util.TEX_PROBES))
def test_oracle_reproduces_the_adversarial_reference_probes(build):
    P = util.load_tex_probe(build)
    mode, mip, aniso = util.TEX_PROBES[build]
    assert list(P["classes"]) == list(texset.CLASSES) and list(P["names"]) == [texset.name8(w, h) for w, h in texset.SHAPES8]
    rows = 0
    for (w, h), name in zip(texset.SHAPES8, P["names"]):
        assert np.array_equal(P["tile_" + name], texset.tile8(w, h)), name              # the committed pixels are the ones texset draws
        tex = texset.texture8(w, h, P["tile_" + name])
        out, _ = orc.texture_sample(tex if mode == 2 else texset.unmipped(tex), P["in_" + name], mode, mip, aniso)
        util.check_colours(out, P["ref_" + name], P["label_" + name], P["classes"], f"{build} {name}")
        assert set(np.unique(P["label_" + name])) == set(range(len(texset.CLASSES))), name      # every class on every texture
        rows += len(out)
    assert rows >= 4000


@pytest.mark.parametrize("w,h", texset.SHAPES8)
def test_texture_chain_matches_numpy_and_the_file_route(w, h, tmp_path):
    """rtxh_texture_mips == the numpy restatement of Texture::load's box filter == rtxh_texture_load of a PNG of the same pixels."""
    tex = texset.texture8(w, h)
    level0 = host.srgb8_to_linear(texset.pixels8(w, h))
    levels, offsets, texels = texset.numpy_chain(level0)
    pow2 = w & (w - 1) == 0 and h & (h - 1) == 0
    assert int(tex.desc["mip_levels"][0]) == levels == (1 + int(np.log2(min(w, h))) if pow2 else 1)
    assert int(tex.desc["mipmapped"][0]) == int(pow2) and (int(tex.desc["width"][0]), int(tex.desc["height"][0])) == (w, h)
    assert tex.desc["mip_offsets"][0, :levels].tolist() == offsets
    assert util.bit_exact(tex.texels, texels) and len(tex.texels) == len(texels)
    for l in range(levels):                                                    # every level the samplers can name has an extent
        assert (w >> l) >= 1 and (h >> l) >= 1 and offsets[l] + (w >> l) * (h >> l) <= len(texels)
    png = str(tmp_path / "t.png")
    host.save_png(png, texset.pack_rgb(texset.pixels8(w, h)))
    loaded = host.load_texture(png)
    assert loaded.desc.tobytes() == tex.desc.tobytes() and util.bit_exact(loaded.texels, tex.texels)
    flat = host.load_texture(png, mipmap_mode=False)
    assert flat.desc.tobytes() == texset.unmipped(tex).desc.tobytes() and util.bit_exact(flat.texels, tex.texels[:w * h])


def test_float_textures_have_the_promised_contents():
    t = texset.float_texture("32x32_special")
    l0 = t.texels[:1024]
    assert np.isinf(l0).any() and (l0 == 0).any() and (l0 == 1).any() and (l0 == np.float32(1e30)).any()
    assert ((l0 != 0) & (np.abs(l0) < np.finfo(np.float32).tiny)).any()
    levels, offsets, texels = texset.numpy_chain(l0.reshape(32, 32, 3))
    assert levels == 6 and util.bit_exact(t.texels, texels)
    c = texset.float_texture("48x48_chain")
    assert int(c.desc["mip_levels"][0]) == 6 and int(c.desc["mipmapped"][0]) == 1
    assert [48 >> l for l in range(6)] == [48, 24, 12, 6, 3, 1]
    assert c.desc["mip_offsets"][0, :6].tolist() == [0, 2304, 2880, 3024, 3060, 3069] and len(c.texels) == 3070


@pytest.mark.parametrize("name", [texset.name8(w, h) for w, h in texset.SHAPES8] + texset.FLOAT_TEXTURES)
def test_sample_sets_keep_every_class_within_the_cost_bound(name):
    tex = texset.all_textures()[name]
    in6, labels = texset.generate(tex, 160, 3)                                  # asserts < 1 % of any class dropped
    again, _ = texset.generate(tex, 160, 3)
    assert in6.dtype == np.float32 and in6.shape[1] == 6 and in6.tobytes() == again.tobytes()
    assert len(in6) >= 2048
    for c in texset.CLASSES:
        assert (labels == c).sum() * 100 > 160 * 99, c
    assert texset.fetch_counts(tex, in6).max() <= texset.MAX_FETCHES
    z = in6[labels == "zero_deriv", 2:]
    assert (z == 0).all()
    t = in6[labels == "tap_counts", 2:].astype(np.float64)
    ext = np.sort(np.stack([np.abs(t[:, [0, 2]]).max(axis=1), np.abs(t[:, [1, 3]]).max(axis=1)]), axis=0)
    taps = np.ceil((ext[1].astype(np.float32) / ext[0].astype(np.float32)))
    assert set(range(1, 18)) <= set(taps.astype(int).tolist()), sorted(set(taps.astype(int).tolist()))
    sp = in6[labels == "special_st", :2]
    assert np.isnan(sp).any() and np.isinf(sp).any() and (np.signbit(sp) & (sp == 0)).any()


def test_batch_oracle_equals_the_single_sample_entry_point():
    import ctypes as C
    tex = texset.texture8(64, 16)
    in6, _ = texset.generate(tex, 16, 9)
    t = orc.OrcTexture()
    C.memmove(C.byref(t.desc), tex.desc.ctypes.data, C.sizeof(orc.RtxTextureDesc))
    t.texels = tex.texels.ctypes.data
    for mode, mip, aniso in texset.CONFIGS.values():
        many, fetches = orc.texture_sample(tex, in6, mode, mip, aniso, threads=3)
        one = np.zeros(3, np.float32)
        for i, r in enumerate(in6):
            orc.lib().orc_texture_sample(C.byref(t), mode, mip, aniso, *[C.c_float(float(x)) for x in r], one.ctypes.data)
            assert util.bit_exact(one, many[i]), (mode, mip, aniso, i)
        assert 0 <= fetches.min() and fetches.max() <= texset.MAX_FETCHES and (mip == 2 and mode == 2 or fetches.min() >= 1)      # an EWA box can be empty


def test_sky_batch_oracle_and_direction_classes():
    import ctypes as C
    dirs, labels = texset.sky_directions(1)
    assert set(labels) == set(texset.SKY_CLASSES)
    for size in (1, 2, 64):
        sky = texset.sky_probe(size)
        out = orc.sky_sample(sky, dirs, threads=3)
        padded = np.zeros((size * size + 1, 3), np.float32); padded[:-1] = sky.reshape(-1, 3)
        one = np.zeros(3, np.float32)
        for i in range(len(dirs)):
            orc.lib().orc_sky_sample(padded.ctypes.data, size, dirs[i].ctypes.data, one.ctypes.data)
            assert util.bit_exact(one, out[i]), (size, i)
        # the inclusive clamp is reached: some direction reads the padding texel (zeros), and acos of |z| > 1 clamps to an end
        assert (out[labels == "index_edges"] == 0).all(axis=1).any(), size
