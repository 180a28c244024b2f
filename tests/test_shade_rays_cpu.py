"""The oracle's shading of caller-supplied rays (oracle/rt_oracle.h orc_shade_rays, orc.OracleScene.shade_rays), without a GPU:
  * on the pinhole rays of every non-heat-map golden it is orc_render_tiles bit for bit (colour, packed pixels, distances, ray counts, work
    counters): one bounce() serves both, so the new entry point inherits the reference pin of tests/test_oracle_golden.py;
  * it reproduces the REAL reference's Raytracer::bounce on the recorded shade probes (tests/golden/unit/shadeprobe_*.npz, made by
    oracle/ref_harness/make_shade_goldens.py from tests/shadeset.py) bit for bit, NaN == NaN;
  * the generated sets are not vacuous: every class is there and reaches the branch it is named for (asserted from the oracle's outputs), and
    at most 2 % of the rays of a class have a tree with a non-finite ray origin (those are kept off the device, test_gpu_shade_rays.py).
lights3 changes what the scene language cannot say (a spot cutoff set to a computed dt, a directional light that is not unit length) and
is oracle-only; every other scene of shadeset.SCENES is reference-pinned."""
import copy
import os

import numpy as np
import pytest

import shadeset
import util

f32 = np.float32
PINHOLE = [n for n in util.GOLDENS if not n.endswith("_heat")]
SEED = 20261018                              # the recorded probes' seed (make_shade_goldens.py)
_out = {}


def same(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    ok = a.view(np.uint32) == b.view(np.uint32)
    if a.dtype == np.float32:
        ok |= np.isnan(a) & np.isnan(b)
    return ok


def shaded(name, seed=SEED):
    """(scene, rays, label, oracle scene, shade_rays(camera=None)) of a generated set, computed once"""
    if (name, seed) not in _out:
        import orc
        sc, rays, label = shadeset.generate(name, seed)
        o = orc.OracleScene(sc)
        _out[(name, seed)] = (sc, rays, label, o, o.shade_rays(rays))
    return _out[(name, seed)]


def with_config(sc, **kw):
    sc = copy.deepcopy(sc)
    for k, v in kw.items():
        sc.config[k] = v
    return sc


def per_ray_counts(sc, rays):
    """(n, 4) ray counts of each ray's own tree: one orc_shade_rays call per ray"""
    import orc
    o = orc.OracleScene(sc)
    return np.array([[o.shade_rays(r[None], threads=1)["stats"][k] for k in ("primary", "shadow", "reflection", "refraction")] for r in rays])


@pytest.mark.parametrize("name", PINHOLE)
def test_pinhole_rays_shade_to_the_tiles_frame(name):
    import orc
    from pyrtx import api
    sc, _ = util.load_golden(name)
    o = orc.OracleScene(sc)
    ref = o.render(threads=8, want_dist=True)
    rays = api.pinhole_rays(sc.camera[0], sc.width, sc.height)
    for cam in (None, np.asarray(sc.camera[0]["position"], f32)):
        out = o.shade_rays(rays, camera=cam)
        for ch in ("rgb", "packed", "dist"):
            bad = ~same(out[ch], ref[ch])
            assert not bad.any(), f"{ch}: {int(bad.sum())} elements differ"
        assert out["stats"] == ref["stats"] and out["work"] == ref["work"]
        assert not out["ray_flags"].any()


def test_camera_rows_and_skipped_rays():
    """camera3 row i is ray i's camera; a zero-direction record is no ray: not counted, outputs untouched"""
    sc, rays, label, o, out = shaded("mirrors")
    flat = rays.reshape(-1, 18)
    live = label.reshape(-1) >= 0
    assert not out["rgb"].reshape(-1, 3)[~live].any() and not out["packed"].reshape(-1)[~live].any() and not out["dist"].reshape(-1)[~live].any()
    assert out["stats"]["primary"] == int(live.sum())
    own = o.shade_rays(flat, camera=flat[:, 0:3])
    assert same(own["rgb"], out["rgb"].reshape(-1, 3)).all() and own["stats"] == out["stats"]
    cams = np.random.default_rng(1).uniform(-5, 5, (len(flat), 3)).astype(f32)
    moved = o.shade_rays(flat, camera=cams)
    k = int(np.flatnonzero(live & ~same(moved["rgb"], own["rgb"]).all(axis=1))[0])           # a ray whose colour depends on its camera
    one = o.shade_rays(flat[k:k + 1], camera=cams[k:k + 1], threads=1)
    assert same(one["rgb"][0], moved["rgb"][k]).all() and not same(one["rgb"][0], own["rgb"][k]).all()


# ---- the reference's own records ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", shadeset.SCRIPTED)
def test_oracle_reproduces_reference_shade_probes(name):
    P = dict(np.load(os.path.join(util.GOLDEN, "unit", f"shadeprobe_{name}.npz")))
    assert os.path.getsize(os.path.join(util.GOLDEN, "unit", f"shadeprobe_{name}.npz")) <= 491883          # the largest file there before these
    sc, rays, label, o, out = shaded(name, int(P["seed"]))
    assert rays.tobytes() == P["rays"].tobytes() and label.tobytes() == P["label"].tobytes(), "the recorded rays are not the generator's"
    assert tuple(P["classes"]) == shadeset.CLASSES
    live = label >= 0
    for ch in ("rgb", "dist"):
        bad = ~same(out[ch], P[ch])
        bad = bad.any(axis=-1) if bad.ndim == 4 else bad
        where = {shadeset.CLASSES[k]: int((label[bad] == k).sum()) for k in np.unique(label[bad])}
        assert not bad.any(), f"{ch}: {int(bad.sum())} rays differ from the reference, by class {where}"
    assert (P["counts"][live][:, 0] == 1).all() and not P["counts"][~live].any()
    for k, cls in enumerate(shadeset.CLASSES):                                       # ray counts: per class (the entry point sums over its rays)
        sub = np.where((label == k)[..., None], rays, f32(0)).astype(f32)
        st = o.shade_rays(sub)["stats"]
        assert [st[x] for x in ("primary", "shadow", "reflection", "refraction")] == P["counts"][label == k].astype(np.int64).sum(axis=0).tolist(), cls


# ---- the generated sets are not vacuous ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", shadeset.SCENES)
def test_every_class_is_there_and_finite_at_level_0(name):
    sc, rays, label, o, out = shaded(name)
    assert rays.shape == (shadeset.V, shadeset.H, shadeset.W, 18) and shadeset.V == 2
    assert np.isfinite(rays[..., :6]).all()
    for v in range(shadeset.V):
        assert set(np.unique(label[v]).tolist()) == set(range(-1, len(shadeset.CLASSES))), f"view {v}"
    assert not rays[label < 0][:, 3:6].any() and np.signbit(rays[label < 0][:, 3:6]).any()
    for k, cls in enumerate(shadeset.CLASSES):
        flagged = (out["ray_flags"][label == k] & 1) != 0
        assert flagged.mean() <= 0.02, f"{cls}: {int(flagged.sum())} of {flagged.size} trees hold a ray with a non-finite origin"


def class_rays(name, cls):
    sc, rays, label, o, out = shaded(name)
    m = label == shadeset.CLASSES.index(cls)
    return sc, o, rays[m], {k: out[k][m] for k in ("rgb", "dist", "ray_flags")}


@pytest.mark.parametrize("name", ["dielectrics", "mirrors"])
def test_origins_reach_deeper_levels_with_cameras_of_their_own(name):
    sc, o, r, out = class_rays(name, "origins")
    assert len(np.unique(r[:, 0:3], axis=0)) > 1000
    st = o.shade_rays(r)["stats"]
    assert st["reflection"] > 1000 and st["shadow"] > st["primary"]                      # lit hits below level 0
    flat = with_config(sc, bounces=0)
    import orc
    deep = ~same(orc.OracleScene(flat).shade_rays(r)["rgb"], out["rgb"]).all(axis=1)     # the colour has a part from depth >= 1 ...
    one_cam = ~same(o.shade_rays(r, camera=r[0, 0:3])["rgb"], out["rgb"]).all(axis=1)    # ... and depends on which origin is the camera
    assert deep.sum() > 1000 and (deep & one_cam).sum() > 1000


@pytest.mark.parametrize("name", ["dielectrics", "mirrors", "lights1"])
def test_critical_takes_the_tir_branch_and_the_spawn_branch(name):
    sc, o, r, _ = class_rays(name, "critical")
    hits, ids = o.trace_closest(r)
    masked = (hits[:, 0] > 0) & (np.asarray(sc.materials["transmittance"])[np.maximum(ids[:, 0], 0)] != 0).any(axis=1)
    refr = per_ray_counts(with_config(sc, bounces=1), r)[:, 3]                          # level 0 alone: 1 = a refraction ray, 0 = total internal reflection
    assert (masked & (refr == 0)).sum() >= 10 and (masked & (refr == 1)).sum() >= 10, (int(masked.sum()), refr.tolist())
    exiting = masked & ((hits[:, 5:8] * r[:, 3:6]).sum(axis=1) > 0)
    assert (exiting & (refr == 0)).any() and (exiting & (refr == 1)).any()
    if name == "dielectrics":                                                            # n_1 > n_2 on entering: TIR from outside
        assert (masked & ~exiting & (refr == 0)).any() and (masked & ~exiting & (refr == 1)).any()


def test_grazing_normal_reaches_exact_dots():
    sc, o, r, _ = class_rays("dielectrics", "grazing_normal")
    hits, _ = o.trace_closest(r)
    hit = hits[:, 0] > 0
    n, d = hits[:, 5:8], r[:, 3:6]
    dot = (d[:, 0] * n[:, 0] + (d[:, 1] * n[:, 1] + d[:, 2] * n[:, 2])).astype(f32)
    assert (hit & (dot == -1)).sum() >= 8 and (hit & (dot == 1)).sum() >= 6
    assert (hit & (dot == 0)).any(), "a tangent hit with dot(d, n) == 0"
    for eps in (f32(2.0 ** -23), f32(1e-7), f32(1e-3), f32(2e-39)):                      # both signs: entering and exiting at grazing incidence
        assert (hit & (dot == -eps)).sum() >= 3 and (hit & (dot == eps)).sum() >= 3, float(eps)
    tiny = np.nextafter(f32(0), f32(1))
    assert (np.abs(r[:, 4]) == tiny).sum() >= 6 and not hit[np.abs(r[:, 4]) == tiny].any()  # one ulp from zero: the distance overflows, a miss
    below = hit & (dot > 0) & (dot < 2e-7)
    assert (np.asarray(sc.materials["transmittance"])[sc.planes["material_id"][0]] != 0).any()      # the floor refracts: these hits take the
    assert (per_ray_counts(with_config(sc, bounces=1), r[below])[:, 3] == 1).all()                  # exiting branch with cos_theta next to 0
    assert (~hit).any()                                                                  # in-plane rays miss the face


def test_non_unit_lengths_hit():
    sc, o, r, _ = class_rays("mirrors", "non_unit")
    length = np.linalg.norm(r[:, 3:6].astype(np.float64), axis=1)
    hits, _ = o.trace_closest(r)
    for want in (1e-3, 0.5, 2.0, 1e3):
        m = np.abs(length / want - 1) < 1e-5
        assert m.sum() >= 30 and (hits[m, 0] > 0).sum() >= 10, want


@pytest.mark.parametrize("name", ["mirrors", "normals"])
def test_differentials_reach_textured_reflective_hits(name):
    sc, o, r, out = class_rays(name, "differentials")
    assert np.isfinite(r[:, :6]).all()
    d = r[:, 6:]
    assert np.isnan(d).any() and np.isinf(d).any() and (d == 0).all(axis=1).any() and (np.abs(d) >= 1e6).any() and ((d != 0) & (np.abs(d) < np.finfo(f32).tiny)).any()
    hits, ids = o.trace_closest(r)
    mats = np.asarray(sc.materials)[np.maximum(ids[:, 0], 0)]
    target = (hits[:, 0] > 0) & (mats["texture_id"] >= 0) & (mats["reflection"] != 0).any(axis=1)
    odd = ~np.isfinite(d).all(axis=1)
    assert (target & odd).sum() >= 20 and (target & ~odd).sum() >= 20
    plain = r.copy(); plain[:, 6:] = f32(1e-3)
    moved = ~same(o.shade_rays(plain)["rgb"], out["rgb"]).all(axis=1)                    # the differentials reach the texture level of detail
    assert (moved & target & odd).sum() >= 10 and (moved & target & ~odd).sum() >= 10, (int((moved & target & odd).sum()), int((moved & target & ~odd).sum()))
    assert np.isfinite(out["rgb"][target & odd]).all(axis=1).any()


def test_poles_and_seam():
    sc, o, r, _ = class_rays("dielectrics", "poles")
    hits, _ = o.trace_closest(r)
    hit = hits[:, 0] > 0
    n = hits[:, 5:8]
    assert (hit & (n[:, 1] >= 1)).sum() >= 2 and (hit & (n[:, 1] <= -1)).sum() >= 1
    assert (hit & (n[:, 0] == 0) & (n[:, 2] < 0)).sum() >= 6


def test_on_surface_origins_are_hit_points():
    sc, rays, label, o, out = shaded("mirrors")
    on = label == shadeset.CLASSES.index("on_surface")
    others = rays[(label >= 0) & ~on]
    hits, _ = o.trace_closest(np.concatenate([others[:, :6], np.zeros((len(others), 12), f32)], axis=1))
    points = {p.tobytes() for p in hits[hits[:, 0] > 0, 2:5]}
    assert all(p.tobytes() in points for p in rays[on][:, 0:3])
    assert np.isfinite(out["rgb"][on]).all(axis=1).any()


def test_lights_reach_nan_and_exactly_zero_contributions():
    import orc
    # lights5: the point light AT the hit point of the first anchor ray: to_light = 0 / 0
    sc, rays, label, o, out = shaded("lights5")
    x, z = shadeset.ANCHORS[0]
    anchor = np.all(rays[..., 0:6] == np.array([x, 3, z, 0, -1, 0], f32), axis=-1)
    assert anchor.sum() == 1 and np.isnan(out["rgb"][anchor]).all()
    assert np.isinf(out["rgb"]).any() and np.isfinite(out["rgb"][label >= 0]).all(axis=1).any()
    # lights3: dt == outer_cutoff exactly at the second anchor: that spot alone, on a floor that only it lights, gives exactly zero
    sc, rays, label, o, out = shaded("lights3")
    x, z = shadeset.ANCHORS[1]
    ray = np.zeros((2, 18), f32); ray[:, 0:6] = (x, 3, z, 0, -1, 0); ray[1, 0] = x - 0.5; ray[1, 2] = z - 0.8       # the second one: inside the cone
    alone = with_config(sc, bounces=0)
    alone.spot_lights = alone.spot_lights[:1].copy(); alone.dir_lights = alone.dir_lights[:0].copy(); alone.ambient = np.zeros(3, f32)
    rgb = orc.OracleScene(alone).shade_rays(ray)["rgb"]
    assert not rgb[0].any() and (rgb[1] > 0).all(), rgb
    wider = copy.deepcopy(alone); wider.spot_lights["outer_cutoff"][0] = np.nextafter(alone.spot_lights["outer_cutoff"][0], f32(-1))
    assert (orc.OracleScene(wider).shade_rays(ray[:1])["rgb"] != 0).any(), "one ulp wider and the anchor is lit"
    assert float(np.linalg.norm(sc.dir_lights["negative_direction"][0])) > 2.9
    # lights0: NaN ambient in one channel
    sc, rays, label, o, out = shaded("lights0")
    hit = (out["dist"] < 1e30) & (label >= 0)                                            # (the grazing hits 2.5e38 away find a black texel: unlit)
    assert np.isnan(out["rgb"][hit][:, 0]).all() and np.isfinite(out["rgb"][hit][:, 1:]).all()


def test_normals_reach_vanishing_and_non_unit_normals():
    sc, rays, label, o, out = shaded("normals")
    live = label >= 0
    hits, ids = o.trace_closest(rays[live])
    mesh = (hits[:, 0] > 0) & (ids[:, 1] == 3)                                           # the ShadeNormals instance
    assert mesh.sum() > 200
    assert np.isnan(hits[mesh, 5:8]).any(axis=1).sum() > 20, "zero normals normalise to NaN"
    opposed = mesh & (hits[:, 2] > -2.0) & (hits[:, 2] < 0.0)                            # quad B: the interpolated normal vanishes on a line in each triangle
    assert np.isnan(hits[opposed, 5:8]).all(axis=1).sum() >= 4 and np.isfinite(hits[opposed, 5:8]).all(axis=1).sum() > 50
    lengths = np.linalg.norm(hits[mesh, 5:8].astype(np.float64), axis=1)
    assert (np.abs(lengths[np.isfinite(lengths)] - 1) < 1e-5).all()
    flat = mesh & (hits[:, 2] > 2.0) & np.isfinite(rays[live][:, 6:]).all(axis=1)          # the quad whose vertices share one uv: x in (2, 4)
    assert (hits[flat, 9] == f32(0.25)).all() and (hits[flat, 10] == f32(0.25)).all()
    assert flat.sum() > 20 and not hits[flat, 11:15].any()                               # every uv equal: zero texture differentials


def only_light(sc, kind, index):
    """the scene with that light alone, no ambient, no bounces"""
    sc = with_config(sc, bounces=0)
    sc.ambient = np.zeros(3, f32)
    for k in ("point_lights", "spot_lights", "dir_lights"):
        setattr(sc, k, getattr(sc, k)[index:index + 1].copy() if k == kind else getattr(sc, k)[:0].copy())
    return sc


def test_degenerate_spot_cones_light_hits():
    import orc
    sc, rays, label, o, out = shaded("lights5")                                          # inner == outer: falloff = x / 0, clamped to 1
    assert sc.spot_lights["inner_cutoff"][0] == sc.spot_lights["outer_cutoff"][0]
    rgb = orc.OracleScene(only_light(sc, "spot_lights", 0)).shade_rays(rays)["rgb"][label >= 0]
    assert (np.isfinite(rgb).all(axis=1) & (rgb > 0).all(axis=1)).sum() >= 100
    for name, k in (("mirrors", 0), ("lights3", 1)):                                     # cutoffs swapped: a negative falloff
        sc, rays, label, o, out = shaded(name)
        assert sc.spot_lights["inner_cutoff"][k] < sc.spot_lights["outer_cutoff"][k]
        rgb = orc.OracleScene(only_light(sc, "spot_lights", k)).shade_rays(rays)["rgb"][label >= 0]
        assert (rgb < 0).any(axis=1).sum() >= 50, name


def test_on_surface_hits_next_to_the_camera():
    sc, o, r, out = class_rays("lights1", "on_surface")
    hits, _ = o.trace_closest(r)
    near = (hits[:, 0] > 0) & (hits[:, 1] < 0.11)
    assert near.sum() >= 12 and np.isfinite(out["rgb"][near]).all()


def test_every_index_of_refraction_is_hit_and_spawns_or_refuses():
    sc, rays, label, o, out = shaded("dielectrics")
    r = rays[label >= 0]
    hits, ids = o.trace_closest(r)
    ior = np.asarray(sc.materials["index_of_refraction"])[np.maximum(ids[:, 0], 0)]
    entering = (hits[:, 5:8] * r[:, 3:6]).sum(axis=1) < 0
    masked = (hits[:, 0] > 0) & (np.asarray(sc.materials["transmittance"])[np.maximum(ids[:, 0], 0)] != 0).any(axis=1)
    b1 = with_config(sc, bounces=1)
    refr = {}
    for key, value, pick in (("one", 1.0, masked), ("one_ulp", np.nextafter(f32(1), f32(2)), masked), ("half", 0.5, masked), ("glass", 1.5, masked),
                             ("1e3_in", 1000.0, masked & entering), ("1e3_out", 1000.0, masked & ~entering), ("zero_in", 0.0, masked & entering)):
        m = pick & (ior == f32(value))
        assert m.sum() >= 5, (key, int(m.sum()))
        refr[key] = per_ray_counts(b1, r[m][:60])[:, 3]                                  # level 0 alone: 1 = a refraction ray
    assert (refr["one"] == 1).all()                                                # eta = 1: k = cos^2, never negative
    assert (refr["one_ulp"] == 1).any()
    assert (refr["1e3_in"] == 1).all() and (refr["1e3_out"] == 0).any()      # into ior 1e3 always, out of it hardly ever
    assert (refr["zero_in"] == 0).mean() > 0.9                                           # eta = 1 / 0: k = -inf (NaN, and a NaN ray, at cos_theta == 1)
    assert (refr["half"] == 0).any() and (refr["half"] == 1).any()             # n_1 > n_2 on entering: both


def test_oracle_reproduces_reference_with_cameras_that_are_no_origins():
    """the camera row of orc_shade_rays apart from the ray's origin, against the reference (Scene::camera.position set per ray)"""
    P = dict(np.load(os.path.join(util.GOLDEN, "unit", "shadeprobe_lights1.npz")))
    sc, rays, label, o, out = shaded("lights1", int(P["seed"]))
    cams = P["camera_table"][P["camera_index"]]
    got = o.shade_rays(rays, camera=cams)
    live = label >= 0
    bad = ~same(got["rgb"], P["rgb_cameras"]).all(axis=-1)
    assert not bad.any(), int(bad.sum())
    assert (~same(P["rgb_cameras"], P["rgb"]).all(axis=-1) & live).sum() > 500             # the camera matters to these rays
    assert got["stats"] == out["stats"]
