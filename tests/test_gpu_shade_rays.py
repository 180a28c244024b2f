"""Colour of caller-supplied rays (rtx_set_rays / rtx_render_rays) against a plain reference: shade_ray and k_resolve (csrc/rtx_shade.h) on
the adversarial scenes and ray classes of tests/shadeset.py — rays with origins of their own (the per-ray camera of Raytracer.cpp:152 at
every depth), critical angles, exact normal dots, non-unit directions, odd differentials, sphere poles, origins on surfaces; exotic
materials, lights and vertex normals.  Bit for bit, NaN == NaN, no tolerance:
  * every scene in every launch shape: rgb, packed pixels and the four ray counts equal the oracle's orc_shade_rays with each ray's own
    origin as its camera; with count_work the work counters too; an AOV call gives the same rgb; pixels of inactive rays keep their fill;
  * one ray view out of two (first_view = 1);
  * the recorded probes (tests/golden/unit/shadeprobe_*.npz): the device against the REAL reference's colours and counts, no oracle between.
A ray whose tree holds a ray with a non-finite origin on the CPU (ray_flags bit 0 of orc_shade_rays) is made inactive before the set goes
to the device: the packet walk is not defined for it below level 0 (ray_is_finite, csrc/rtx_trace.h).  test_shade_rays_cpu.py caps their share."""
import os

import numpy as np
import pytest

import shadeset
import util
from test_gpu_parity import MODES

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = 20261018
STATS = ("primary", "shadow", "reflection", "refraction")
WORK = ("closest_rays", "any_rays", "tlas_nodes_closest", "tlas_nodes_any", "blas_nodes_closest", "blas_nodes_any", "instances_closest", "instances_any",
        "tri_tests_closest", "tri_tests_any", "shaded_hits", "sky_lookups", "texel_fetches", "rays_spawned")
SHAPES = {"default": {}, "serial": MODES["serial"], "serial_lane": MODES["serial_lane"], "simple": {"simple_trace": True},
          "packet_closest": MODES["packet_closest"], "cull": MODES["serial_cull"], "fuse": {}, "count_work": {"count_work": True}}
_want = {}


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def device_set(name, seed=SEED):
    """(scene, rays for the device, live mask, the oracle's shading of exactly those rays), computed once"""
    if (name, seed) not in _want:
        import orc
        sc, rays, label = shadeset.generate(name, seed)
        o = orc.OracleScene(sc)
        flagged = (o.shade_rays(rays)["ray_flags"] & 1) != 0
        rays = rays.copy()
        rays[flagged, 3:6] = 0                                       # never sent to a GPU
        want = o.shade_rays(rays)
        assert not want["ray_flags"].any() and np.isfinite(rays[..., :6]).all()
        _want[(name, seed)] = (sc, rays, (label >= 0) & ~flagged, want)
    return _want[(name, seed)]


def assert_same(got, want, what):
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if got.dtype == np.float32:
        bad &= ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ"


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", shadeset.SCENES)
def test_shaded_rays_equal_the_oracle(api, name, shape, monkeypatch):
    import torch
    if shape == "fuse":
        monkeypatch.setenv("RTX_FUSE_SHADE", "1")                    # read in rtx_create
    flags = SHAPES[shape]
    sc, rays, live, want = device_set(name)
    V, H, W = live.shape
    r = api.Renderer(sc)
    rgb = torch.full((V, H, W, 3), -5.5, dtype=torch.float32, device="cuda"); packed = torch.full((V, H, W), -9, dtype=torch.int32, device="cuda")
    r.render_rays_into(rgb, packed, torch.from_numpy(rays).cuda(), **flags)
    torch.cuda.synchronize()
    stats, work = r.stats()
    got_rgb = rgb.cpu().numpy(); got_packed = packed.cpu().numpy()
    assert_same(got_rgb[live], want["rgb"][live], "rgb")
    assert_same(got_packed.view(np.uint32)[live], want["packed"][live], "packed")
    assert (got_rgb[~live] == f32(-5.5)).all() and (got_packed[~live] == -9).all(), "a pixel without a ray was written"
    assert {k: stats[k] for k in STATS} == {k: want["stats"][k] for k in STATS}
    assert stats["primary"] == int(live.sum())
    if flags.get("count_work"):
        assert {k: work[k] for k in WORK} == {k: want["work"][k] for k in WORK}
    r.set_rays(rays)
    aov = r.render_rays(aovs=("depth", "material_id"), **flags)      # the AOV kernels shade the same colour
    assert_same(aov["rgb"][live], want["rgb"][live], "AOV call rgb")
    assert_same(aov["depth"].reshape(live.shape)[live], want["dist"][live], "depth")
    assert {k: aov["stats"][k] for k in STATS} == {k: want["stats"][k] for k in STATS}
    r.close()


@pytest.mark.parametrize("name", ["dielectrics", "mirrors"])
def test_second_ray_view_alone(api, name):
    """pixel = view * view_pixels + ..: the second of two ray views on its own, whose rays' origins are not the first view's"""
    import orc
    sc, rays, live, want = device_set(name)
    r = api.Renderer(sc)
    r.set_rays(rays)
    out = r.render_rays(first_view=1, view_count=1)
    r.close()
    assert out["rgb"].shape[0] == 1
    assert_same(out["rgb"][0][live[1]], want["rgb"][1][live[1]], "rgb of view 1")
    assert_same(out["packed"][0][live[1]], want["packed"][1][live[1]], "packed of view 1")
    one = orc.OracleScene(sc).shade_rays(rays[1])["stats"]
    assert {k: out["stats"][k] for k in STATS} == {k: one[k] for k in STATS}
    assert not np.array_equal(rays[0][..., 0:3], rays[1][..., 0:3])


@pytest.mark.parametrize("shape", ["default", "serial"])
@pytest.mark.parametrize("name", shadeset.SCRIPTED)
def test_device_reproduces_reference_shade_probes(api, name, shape):
    P = dict(np.load(os.path.join(util.GOLDEN, "unit", f"shadeprobe_{name}.npz")))
    sc, rays, live, want = device_set(name, int(P["seed"]))
    assert rays.tobytes() == P["rays"].tobytes(), "no recorded ray had to be kept off the device"
    r = api.Renderer(sc)
    r.set_rays(P["rays"])
    out = r.render_rays(**SHAPES[shape])
    r.close()
    bad = out["rgb"].view(np.uint32) != P["rgb"].view(np.uint32)
    bad &= ~(np.isnan(out["rgb"]) & np.isnan(P["rgb"]))
    bad = bad.any(axis=-1) & live
    where = {shadeset.CLASSES[k]: int((P["label"][bad] == k).sum()) for k in np.unique(P["label"][bad])}
    assert not bad.any(), f"{int(bad.sum())} rays differ from the reference, by class {where}"
    assert [out["stats"][k] for k in STATS] == P["counts"].astype(np.int64).sum(axis=(0, 1, 2)).tolist()
