"""Scenes for the deepest recursion the render path supports: RTX_MAX_LEVELS = 12 levels (bounces 0 .. 11, csrc/rtx_limits.h), with
levels that GROW with depth — the case alloc_queues sizes level d's queue for (`P << d` rays: every hit spawns two children) — and
with more lights than any bit mask is wide.  Plain scripts in the scene language of oracle/ref_harness/refdump.cpp, assembled by
pyrtx.assemble.scene_from_script (accel="sbvh", mip_filter=1, texture_mode=2); the oracle supplies every expected frame.

shells(w=32, h=32)   one tile.  The camera (0.3 0.5 -1) sits inside six concentric glass spheres at the origin, radii 3, 5, 8, 13, 21, 34,
                     each with transmittance 0.9, reflection 0.4 and ior 1.1 / 1.2 / 1.3 by index; a glass Cube.obj (its texture kept) at
                     0.5 0 1.5; one point light, one directional light, the synthetic sky at a quarter of its brightness.  Every primary ray hits glass from inside a sphere, so level 1 holds
                     exactly two rays per pixel, and nearly every ray of every level hits glass again.
hall(w=64, h=32, lights=3)
                     two tiles.  A closed room: floor, ceiling and back wall are planes with reflection 0.8 .. 0.9; three glass spheres, a
                     glass Cube.obj and a reflective Torus.obj (two instances: the default plan hands levels >= 2 to the per-lane kernels);
                     no texture, every diffuse colour non-zero, so every hit casts one shadow ray per light.  lights=3: one point, one spot,
                     one directional light.  lights=33: 11 + 11 + 11 of them at seeded positions; the light list is all that differs.

Per-level ray counts the oracle gave where this was written (level d = stats at bounces d minus stats at bounces d - 1; reflection +
refraction rays; tests/test_deep_levels_cpu.py asserts the CONDITIONS these show, not the figures):
  shells 32x32   level 1 .. 11:  2048 3955 7448 14535 28166 55406 106279 208649 399145 781121 1489010 (x 1.87 .. 1.97 per level)
                 shadow rays of level 11: 2 947 308; no NaN or inf pixel
  hall 64x32     level 1 .. 11:  2274 2724 3266 3920 4711 5711 6929 8442 10312 12679 15601
                 of which refraction: 226 450 583 654 792 1001 1218 1513 1870 2370 2923; with 33 lights 33 shadow rays per hit (514 767 at level 11)
"""
import copy
import os

import numpy as np

import util
from pyrtx import assemble

DATA = os.path.join(util.GOLDEN, "meshes")
MAX_BOUNCES = 11                              # RTX_MAX_LEVELS - 1
RADII = (3, 5, 8, 13, 21, 34)
STATS = ("primary", "reflection", "refraction", "shadow")

_scenes, _frames, _counts = {}, {}, {}


def _shells_script(w, h):
    s = [f"size {w} {h}", f"bounces {MAX_BOUNCES}", "camera 0.3 0.5 -1 0 0 0 1", "ambient 0.005 0.005 0.006"]
    for i, r in enumerate(RADII):
        s += [f"sphere 0 0 0 {r}", f"matset sphere:{i} transmittance 0.9 0.9 0.9", f"matset sphere:{i} reflection 0.4 0.4 0.4",
              f"matset sphere:{i} ior {(1.1, 1.2, 1.3)[i % 3]}"]
    s += ["mesh ./Data/Cube.obj 0.5 0 1.5", "matset mesh:0:0 transmittance 0.9 0.9 0.9", "matset mesh:0:0 reflection 0.4 0.4 0.4", "matset mesh:0:0 ior 1.5",
          "point 2 1.8 1.6 1 2 -2", "dir 0.02 0.025 0.03 0.3 -1 0.4"]
    return "\n".join(s) + "\n"


def _hall_lights(lights):
    if lights == 3:
        return ["point 5 5 4.5 0 3 2", "spot 8 8 9 -2 3.5 1 0.3 -1 0.5 80 50", "dir 0.2 0.2 0.18 0.2 -1 0.3"]
    assert lights % 3 == 0
    n = lights // 3
    rng = np.random.default_rng(33)
    out = []
    for _ in range(n):
        p = rng.uniform((-4.5, 1.0, -1.5), (4.5, 3.8, 8.5))
        out.append("point 0.8 0.8 0.7 %.4f %.4f %.4f" % tuple(p))
    for _ in range(n):
        p = rng.uniform((-4.5, 2.0, -1.5), (4.5, 3.8, 8.5)); d = rng.uniform((-0.6, -1.0, -0.6), (0.6, -0.5, 0.6))
        out.append("spot 1.5 1.5 1.6 %.4f %.4f %.4f %.4f %.4f %.4f 90 50" % (tuple(p) + tuple(d)))
    for _ in range(n):
        d = rng.uniform((-0.7, -1.0, -0.7), (0.7, -0.4, 0.7))
        out.append("dir 0.03 0.03 0.025 %.4f %.4f %.4f" % tuple(d))
    return out


def _hall_script(w, h, lights):
    half_pi = "1.5707963"
    s = [f"size {w} {h}", f"bounces {MAX_BOUNCES}", "camera 0 1 -2 0 0 0 1", "ambient 0.05 0.05 0.05",
         "plane 0 -1 0",                                             # floor
         "plane_axis_angle 0 4 0 1 0 0 3.14159265",                  # ceiling
         f"plane_axis_angle 0 0 9 1 0 0 -{half_pi}",                 # back wall
         "matset plane:0 reflection 0.8 0.8 0.8", "matset plane:1 reflection 0.85 0.85 0.85", "matset plane:2 reflection 0.9 0.9 0.9",
         "sphere -2.2 0.2 4 1.2", "sphere 0.3 0 2.5 1", "sphere 2.6 0.8 5 1.4"]
    for i, ior in enumerate((1.5, 1.3, 1.2)):
        s += [f"matset sphere:{i} transmittance 0.9 0.95 0.9", f"matset sphere:{i} reflection 0.3 0.3 0.3", f"matset sphere:{i} ior {ior}"]
    s += ["mesh_axis_angle ./Data/Cube.obj -0.8 0 6 0 1 0 0.6", "mesh_axis_angle ./Data/Torus.obj 1.5 2.4 6.5 1 0 0 0.9",
          "matset mesh:0:0 notexture", "matset mesh:0:0 transmittance 0.9 0.9 0.95", "matset mesh:0:0 reflection 0.3 0.3 0.3", "matset mesh:0:0 ior 1.4",
          "matset mesh:1:0 diffuse 0.2 0.3 0.8", "matset mesh:1:0 reflection 0.7 0.7 0.7"]
    return "\n".join(s + _hall_lights(lights)) + "\n"


def _scene(key, text):
    if key not in _scenes:
        _scenes[key] = assemble.scene_from_script(text, DATA, accel="sbvh", mip_filter=1, texture_mode=2)
    return copy.deepcopy(_scenes[key])


def shells(w=32, h=32):
    sc = _scene(("shells", w, h), _shells_script(w, h))
    # twelve levels of Ks + Kt = 1.3 amplify what the last rays see: the sky at a quarter (an exact scaling) keeps the packed pixels off the clamp
    sc.sky = (sc.sky * np.float32(0.25)).astype(np.float32)
    return sc


def hall(w=64, h=32, lights=3):
    return _scene(("hall", w, h, lights), _hall_script(w, h, lights))


def light_count(sc):
    return len(sc.point_lights) + len(sc.spot_lights) + len(sc.dir_lights)


def with_bounces(sc, b):
    s = copy.deepcopy(sc)
    s.config["bounces"] = b
    return s


def with_camera(sc, cam):
    s = copy.deepcopy(sc)
    s.camera = np.array([cam], dtype=sc.camera.dtype)
    return s


def _key(sc):
    """what an oracle frame of these scenes depends on: the scene (its spheres tell shells from hall), size, bounces, lights, camera, materials"""
    return (len(sc.spheres), sc.width, sc.height, int(sc.config["bounces"][0]), light_count(sc), sc.camera.tobytes(), np.ascontiguousarray(sc.materials).tobytes())


def oracle_frame(sc, threads=8):
    """The oracle's frame of sc (rgb, packed, stats, work), rendered once per (scene, size, bounces, lights, camera); read-only."""
    k = _key(sc)
    if k not in _frames:
        import orc
        out = orc.OracleScene(sc).render(threads=threads)
        out["rgb"].setflags(write=False); out["packed"].setflags(write=False)
        _frames[k] = out
    return _frames[k]


def level_counts(sc):
    """Per level 0 .. bounces of sc: {"primary", "reflection", "refraction", "shadow", "hits"} — the rays TRACED at that level (level d's
    reflection rays are spawned by the hits of level d - 1) and the hits shaded there, as differences of the oracle's counters at bounces d and d - 1."""
    k = _key(sc)
    if k not in _counts:
        top = int(sc.config["bounces"][0])
        rows, prev = [], None
        for b in range(top + 1):
            f = oracle_frame(with_bounces(sc, b))
            cur = dict({n: int(f["stats"][n]) for n in STATS}, hits=int(f["work"]["shaded_hits"]))
            rows.append({n: cur[n] - (prev[n] if prev else 0) for n in cur})
            prev = cur
        _counts[k] = rows
    return _counts[k]


def level_rays(sc):
    """rays traced at each level: the primary rays at level 0, reflection + refraction rays below"""
    return [r["primary"] + r["reflection"] + r["refraction"] for r in level_counts(sc)]
