"""Seeded adversarial scenes and primary rays for the shading kernels (shade_ray / k_resolve, csrc/rtx_shade.h), plain numpy; the oracle
supplies the hit points the surface starts begin at.

generate(scene_name, seed) -> (scene_io.Scene, rays (V, H, W, 18) float32, label (V, H, W) int8: index into CLASSES, -1 = no ray there).
Every scene is 64x48 with V = 2 ray views; rays are aimed with float64 geometry and rounded to float32; every origin and direction is
finite (NaN / inf appear in the differentials of one class only); records with a zero direction (no ray) are scattered through both views.

Scenes (SCENES; script(name) is the text in the scene language of oracle/ref_harness/refdump.cpp that the reference can be driven with, EDITS
what is changed after assembly where that language cannot say it — such scenes are oracle-only, the others are in SCRIPTED).  Common
geometry: a floor plane y = -1 (exact axis normal), a back wall, a sphere inside a sphere, a glass ball, an unrotated cube, two instances
of one torus.  All use the anisotropic mip filter: its work per sample is bounded whatever the differentials are.
  dielectrics  bounces 3: ior exactly 1 (floor), 1 + 1 ulp (inner sphere), 0.5 (outer sphere: n_1 > n_2 on entering), 1e3 (cube), 0 (tori);
               transmittance with one non-zero component, above 1, negative
  mirrors      bounces 5: floor and ceiling are facing mirrors; reflection with zero components / one component (cube), above 1 (outer
               sphere), negative (tori); diffuse exactly 0 on a reflective wall; a negative diffuse (ceiling); a spot with the cutoffs swapped
  lights0      bounces 0: no light, a NaN ambient component
  lights1      bounces 1: one directional light, zero ambient
  lights5      bounces 1: a point light exactly at a hit point (ANCHORS[0]), one in the floor's plane (huge colour), one behind the floor (negative
               colour), a spot with inner_cutoff == outer_cutoff, a directional light with an infinite colour component; zero ambient
  lights3      bounces 1, oracle-only (the computed cutoff and the light that is not unit length need EDITS): a spot whose outer_cutoff is
               exactly dt of the hit at ANCHORS[1], a directional light of length 3; also a spot with the cutoffs swapped; negative ambient
  normals      bounces 3: tests/golden/meshes/ShadeNormals.obj (zero, opposed and non-unit vertex normals, every uv equal) in front

Ray classes (CLASSES):
  origins         every ray its own origin: an orthographic grid and random origins around the scene (the per-ray camera at depth >= 1)
  critical        incidence at the critical angle of the glass ball from inside (and of the ior 0.5 sphere from outside) and 1, 2, 4, ..
                  4096 ulps of cos_theta to either side
  grazing_normal  axis-aligned rays on the floor and the cube's faces: dot(d, n) exactly -1 and +1, 0 (in the face's plane: a miss; a sphere
                  tangent: a hit), +-2^-23, +-1e-7, +-1e-3 and +-2e-39 on the floor from above and from below (one ulp from zero, +-1.4e-45, is
                  generated too but its hit distance overflows: a miss); sphere tangents; the straight-down rays onto ANCHORS; rays onto the
                  points of ShadeNormals.obj where the interpolated normal is exactly zero
  non_unit        direction lengths 1e-3, 0.5, 2, 1e3
  differentials   zero, 1e6, subnormal, NaN and inf differentials (columns 6..17) on textured, reflective targets
  poles           sphere hits at normal.y = +-1 (from outside and inside) and on the seam normal.x = 0, normal.z < 0
  on_surface      origins at the fp32 hit point of an earlier ray, fresh directions; twelve start under the overhang of the glass ball and hit it
                  0.02 .. 0.1 away
"""
import os

import numpy as np

import util
from pyrtx import assemble

f32 = np.float32
DATA = os.path.join(util.GOLDEN, "meshes")
W, H, V = 64, 48, 2
CLASSES = ("origins", "critical", "grazing_normal", "non_unit", "differentials", "poles", "on_surface")
SCENES = ("dielectrics", "mirrors", "lights0", "lights1", "lights5", "lights3", "normals")
ANCHORS = ((0.0, 4.0), (1.0, 3.0))         # (x, z): the ray straight down from (x, 3, z) hits the floor at exactly (x, -1, z)
ULPS = (0,) + tuple(s * (1 << k) for k in range(13) for s in (1, -1))

SPHERES = (((-2.0, 0.5, 5.0), 1.5), ((-2.0, 0.5, 5.0), 0.6), ((2.5, 0.0, 4.0), 1.0))      # outer, inner, glass ball
CUBE = (0.5, 0.0, 8.0)                      # Cube.obj: +-1 around it, unrotated
NORMALS_AT = (0.0, -0.5, 6.5)               # where the normals scene puts ShadeNormals.obj (x -4 .. 4, y 0 .. 2 in the mesh's z = 0 plane)
GEOMETRY = ["size 64 48", "camera 0 1 -4 0 0 0 1",
            "plane 0 -1 0", "plane_axis_angle 0 0 12 1 0 0 -1.5707963",
            "sphere -2 0.5 5 1.5", "sphere -2 0.5 5 0.6", "sphere 2.5 0 4 1",
            "mesh ./Data/Cube.obj 0.5 0 8", "mesh_axis_angle ./Data/Torus.obj 3 2 8 1 0 0 0.9", "mesh_axis_angle ./Data/Torus.obj -3.5 2.5 9 0 0 1 1.2",
            "matset plane:0 texture ./Data/Floor.png", "matset plane:0 reflection 0.3 0.3 0.3",
            "matset sphere:2 transmittance 0.9 0.95 0.9", "matset sphere:2 ior 1.5"]
ONE_PLUS_ULP = "1.00000012"                 # float32(1) + 1 ulp
_SCRIPTS = {
    "dielectrics": ["bounces 3", "ambient 0.1 0.1 0.1", "point 20 20 20 1 6 1", "dir 0.6 0.6 0.5 0.2 -1 0.3",
                    "matset plane:0 transmittance 0.2 0.2 0.2", "matset plane:0 ior 1",
                    "matset sphere:0 transmittance 0 0.8 0", "matset sphere:0 ior 0.5",
                    "matset sphere:1 transmittance 1.5 2 1.2", "matset sphere:1 ior " + ONE_PLUS_ULP,
                    "matset mesh:0:0 transmittance -0.5 0.3 0.2", "matset mesh:0:0 ior 1000", "matset mesh:0:0 reflection 0.3 0.3 0.3",
                    "matset mesh:1:0 transmittance 0.5 0.5 0.5", "matset mesh:1:0 ior 0"],
    "mirrors": ["bounces 5", "plane_axis_angle 0 5 0 1 0 0 3.14159265", "ambient 0.1 0.1 0.1", "point 15 15 15 0 3 2",
                "spot 30 30 30 -3 4.5 0 0.5 -1 0.8 70 40",
                "matset plane:0 reflection 0.9 0.9 0.9", "matset plane:2 reflection 0.9 0.9 0.9", "matset plane:2 diffuse -0.5 0.2 -0.1",
                "matset plane:1 diffuse 0 0 0", "matset plane:1 reflection 0.8 0.8 0.8",
                "matset mesh:0:0 transmittance 0 0 0", "matset mesh:0:0 reflection 0 0.7 0",
                "matset sphere:0 reflection 1.5 2 1.2", "matset mesh:1:0 reflection -0.5 -0.2 0.3"],
    "lights0": ["bounces 0", "nolights", "ambient nan 0.2 0.1"],
    "lights1": ["bounces 1", "ambient 0 0 0", "dir 0.9 0.8 0.7 0.3 -1 0.2"],
    "lights5": ["bounces 1", "ambient 0 0 0", "point 5 5 5 0 -1 4", "point 1e30 1e30 1e30 6 -1 2", "point -1 -2 -0.5 0 -3 5",
                "spot 20 20 20 -1 4 3 0.2 -1 0.3 40 40", "dir inf 1e30 1 0.1 -1 0.1"],
    "lights3": ["bounces 1", "ambient -0.2 -0.1 -0.3", "spot 30 30 30 0 4 1 0 -1 0.1 30 60", "spot 20 25 30 -2 4 6 0.1 -1 -0.2 70 40",
                "dir 0.5 0.6 0.7 0.2 -1 0.3"],
    "normals": ["bounces 3", "ambient 0.1 0.1 0.1", "mesh ./Data/ShadeNormals.obj %g %g %g" % NORMALS_AT, "point 20 20 20 0 5 0", "dir 0.5 0.5 0.5 0.1 -1 0.4"],
}


def _dot(a, b):                             # the oracle's vdot, in float32
    return f32(a[0] * b[0]) + f32(f32(a[1] * b[1]) + f32(a[2] * b[2]))


def _edit_lights3(sc):
    """What the script language cannot say: outer_cutoff of spot 0 = dt at the hit point of ANCHORS[1], bit for bit (Raytracer.cpp:172-178 in
    the oracle's operation order); a directional light that is not unit length."""
    p = np.array([ANCHORS[1][0], -1.0, ANCHORS[1][1]], f32)
    to_light = (sc.spot_lights["position"][0].astype(f32) - p).astype(f32)
    d = np.sqrt(_dot(to_light, to_light), dtype=f32)
    to_light = (to_light * f32(f32(1.0) / d)).astype(f32)
    sc.spot_lights["outer_cutoff"][0] = _dot(to_light, sc.spot_lights["negative_direction"][0].astype(f32))
    sc.dir_lights["negative_direction"][0] = (sc.dir_lights["negative_direction"][0] * f32(3.0)).astype(f32)


EDITS = {"lights3": _edit_lights3}
SCRIPTED = tuple(n for n in SCENES if n not in EDITS)
_scenes, _sets = {}, {}


def script(name):
    return "\n".join(GEOMETRY + _SCRIPTS[name]) + "\n"


def scene(name):
    if name not in _scenes:
        sc = assemble.scene_from_script(script(name), DATA, accel="sbvh", mip_filter=1, texture_mode=2)
        if name in EDITS:
            EDITS[name](sc)
        _scenes[name] = sc
    return _scenes[name]


# ---- rays --------------------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _step(x, k):
    """the float32 k ulps away from x (k steps of the bit pattern: away from zero for k > 0)"""
    return np.uint32(int(f32(x).view(np.uint32)) + k).view(f32)


def _od(o, d):
    return np.concatenate([np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)], axis=1)


def _aimed(o, target):
    d = np.asarray(target, np.float64) - np.asarray(o, np.float64)
    return _od(o, d / np.linalg.norm(d, axis=-1, keepdims=True))


def _small_differentials(rng, n):
    return np.concatenate([rng.uniform(-0.01, 0.01, (n, 6)), rng.uniform(-0.002, 0.002, (n, 6))], axis=1)


def _targets(rng, n):
    """points on or near the objects"""
    c = np.array([s[0] for s in SPHERES] + [CUBE, (3.0, 2.0, 8.0), (-3.5, 2.5, 9.0), (0.0, 0.5, 6.5)])
    return c[rng.integers(len(c), size=n)] + rng.uniform(-1.0, 1.0, (n, 3))


def _random_aimed(rng, n):
    o = rng.uniform((-7.0, -0.8, -3.0), (7.0, 4.8, 11.0), (n, 3))
    return _aimed(o, _targets(rng, n))


def _origins(rng, n):
    g = n // 2
    k = np.arange(g)
    nx = 32
    o = np.stack([-6.0 + 12.0 * (k % nx) / (nx - 1), -0.9 + 5.4 * (k // nx) / max(1, (g - 1) // nx), np.full(g, -3.0)], axis=1)
    d = np.array([0.05, -0.08, 1.0]); d /= np.linalg.norm(d)
    grid = np.concatenate([_od(o, np.broadcast_to(d, o.shape)), np.zeros((g, 12))], axis=1)
    grid[:, 6] = 12.0 / (nx - 1); grid[:, 10] = 5.4 / max(1, (g - 1) // nx)          # dO_dx, dO_dy of the grid; dD = 0
    rnd = _random_aimed(rng, n - g)
    return np.concatenate([grid, np.concatenate([rnd, _small_differentials(rng, len(rnd))], axis=1)])


def _critical_at(rng, centre, r, eta, inside, points):
    """eta = n_1 / n_2 > 1 of the crossing; cos_theta at the critical angle is sqrt(1 - 1 / eta^2)"""
    out = []
    c = np.asarray(centre, np.float64)
    cos_c = f32(np.sqrt(1.0 - 1.0 / (eta * eta)))
    for _ in range(points):
        n = _unit(rng, 1)[0]; n[1] = abs(n[1]) + 0.3; n /= np.linalg.norm(n)          # upper half: nothing between the origin and the sphere
        t = np.cross(n, _unit(rng, 1)[0]); t /= np.linalg.norm(t)
        for k in ULPS:
            cos = float(_step(cos_c, k))
            sin = np.sqrt(max(0.0, 1.0 - cos * cos))
            d = (cos if inside else -cos) * n + sin * t
            o = c + r * n - d * (r * cos if inside else 1.0)
            out.append(np.concatenate([o, d]))
    return np.array(out)


def _critical(rng, name):
    c2, r2 = SPHERES[2]
    rays = [_critical_at(rng, c2, r2, 1.5, True, 3)]
    if name == "dielectrics":
        c0, r0 = SPHERES[0]
        rays.append(_critical_at(rng, c0, r0, 2.0, False, 2))                           # entering ior 0.5: n_1 / n_2 = 2
    return np.concatenate(rays)


def _grazing(rng):
    out = [((x, 3.0, z), (0.0, -1.0, 0.0)) for x, z in ANCHORS]
    tiny = float(np.nextafter(f32(0), f32(1)))
    for x, z in ((-4.0, 1.0), (4.5, 6.0), (0.3, 10.0)):
        out.append(((x, 3.0, z), (0.0, -1.0, 0.0)))                                     # floor, dot == -1
        out.append(((x, -3.0, z), (0.0, 1.0, 0.0)))                                     # from below, dot == +1
        # grazing, half a unit above the floor (dot < 0) and below it (dot > 0: an exiting hit with cos_theta next to 0): dot(d, n) = -+eps for
        # 2^-23, 1e-7, 1e-3 and 2e-39, about the smallest whose hit distance 0.5 / eps is still finite; the dot one ulp from zero (1.4e-45)
        # and the parallel rays +-0 give an infinite or NaN distance: misses
        for eps in (1.1920929e-07, 1e-7, 1e-3, 2e-39, tiny, 0.0):
            out.append(((x - 6.0, -0.5, z), (1.0, -eps, 0.0)))
            out.append(((x - 6.0, -1.5, z), (1.0, eps, 0.0)))
    cx, cy, cz = CUBE
    for ax in range(3):
        for sgn in (1.0, -1.0):
            e = np.zeros(3); e[ax] = sgn
            off = np.array([0.3, 0.4, -0.2]); off[ax] = 0.0
            out.append((np.array(CUBE) + 4.0 * e + off, -e))                            # head-on from outside, dot == -1
            out.append((np.array(CUBE) + off * 0.5, e))                                 # from inside, dot == +1
            inplane = np.array(CUBE) + e; u = np.zeros(3); u[(ax + 1) % 3] = 1.0
            out.append((inplane - 3.0 * u, u))                                          # in the face's plane, dot == 0
    (sx, sy, sz), r = SPHERES[2]
    x_t = f32(sx + r)
    for k in (0, 1, 2, -1, -2):                                                         # tangents of the glass ball, and a few ulps inside / outside
        out.append(((float(_step(x_t, k)), sy, sz - 3.0), (0.0, 0.0, 1.0)))
    out.append(((sx - 3.0, sy + r, sz), (1.0, 0.0, 0.0)))
    # ShadeNormals.obj at NORMALS_AT, quad B (opposed vertex normals): points where the barycentric weight of the odd vertex is exactly 0.5, so
    # that the interpolated normal is exactly zero; axis-aligned rays starting 1 / 16 in front (in the other scenes they simply go on)
    for lx, ly in ((-1.5, 1.5), (-1.75, 1.25), (-1.25, 1.75), (-0.5, 0.5), (-0.75, 0.25), (-0.25, 0.75)):
        out.append(((NORMALS_AT[0] + lx, NORMALS_AT[1] + ly, NORMALS_AT[2] - 0.0625), (0.0, 0.0, 1.0)))
    return np.array([np.concatenate([np.asarray(o, np.float64), np.asarray(d, np.float64)]) for o, d in out])


def _under_ball():
    """straight down onto the floor from under the overhang of the glass ball, which touches the floor: from the hit points, straight up, the ball
    is 0.02 .. 0.1 away (on_surface: a hit next to a camera that lies on a surface)"""
    (sx, sy, sz), r = SPHERES[2]
    out = []
    for k in range(12):
        rho, phi = 0.2 + 0.02 * k, k * np.pi / 6
        gap = r - np.sqrt(r * r - rho * rho)
        out.append((sx + rho * np.cos(phi), sy - r + 0.5 * gap, sz + rho * np.sin(phi), 0.0, -1.0, 0.0))
    return np.array(out)


def _non_unit(rng, n):
    base = _random_aimed(rng, n)
    scale = np.array([1e-3, 0.5, 2.0, 1e3])[np.arange(n) % 4]
    base[:, 3:6] *= scale[:, None]
    return base


def _differentials(rng, n):
    """aimed at the textured, reflective floor and at the cube; returns all 18 columns"""
    m = n // 2
    o = rng.uniform((-5.0, 0.5, -2.0), (5.0, 4.5, 6.0), (n, 3))
    tg = np.concatenate([np.stack([rng.uniform(-5, 5, m), np.full(m, -1.0), rng.uniform(0, 10, m)], axis=1), np.array(CUBE) + rng.uniform(-0.9, 0.9, (n - m, 3))])
    od = _aimed(o, tg)
    diff = np.zeros((n, 12))
    kinds = np.arange(n) % 8
    sign = rng.choice([-1.0, 1.0], size=(n, 12))
    diff[kinds == 1] = 1e6 * sign[kinds == 1]
    diff[kinds == 2] = 1e-40 * sign[kinds == 2]
    diff[kinds == 3] = np.nan
    diff[kinds == 4] = np.inf * sign[kinds == 4]
    diff[kinds == 5] = _small_differentials(rng, int((kinds == 5).sum())); diff[kinds == 5, 6:12] = np.nan        # only dD is NaN
    diff[kinds == 6] = _small_differentials(rng, int((kinds == 6).sum())); diff[kinds == 6, 0:3] = np.inf         # only dO_dx is inf
    diff[kinds == 7] = 1e6 * rng.uniform(-1, 1, (int((kinds == 7).sum()), 12))
    return np.concatenate([od, diff], axis=1)


def _poles(rng):
    out = []
    for (c, r), inner in ((SPHERES[0], 0.7), (SPHERES[2], 0.0)):
        cx, cy, cz = c
        out.append(((cx, cy + 4.0, cz), (0, -1, 0)))                                   # top pole from outside
        out.append(((cx, cy - inner, cz), (0, -1, 0)))                                 # bottom pole from inside
        out.append(((cx, cy + inner, cz), (0, 1, 0)))                                  # top pole from inside
        for dy in (0.0, 0.3, -0.3, 0.9 * r, -0.6 * r):                                 # the seam: normal.x == 0, normal.z < 0
            out.append(((cx, cy + dy, cz - 4.0), (0, 0, 1)))
            for k in (1, -1):
                out.append(((float(_step(f32(cx), k * (1 if cx > 0 else -1))), cy + dy, cz - 4.0), (0, 0, 1)))
    return np.array([np.concatenate([np.asarray(o, np.float64), np.asarray(d, np.float64)]) for o, d in out])


N_INACTIVE, N_SURFACE, N_NON_UNIT, N_DIFF = 520, 320, 160, 240


def generate(name, seed=0, threads=8):
    """see the module doc"""
    key = (name, seed)
    if key in _sets:
        return _sets[key]
    import orc
    sc = scene(name)
    rng = np.random.default_rng(seed)
    parts = {}

    def with_diff(od):
        return np.concatenate([od, _small_differentials(rng, len(od))], axis=1)
    parts["critical"] = with_diff(_critical(rng, name))
    parts["grazing_normal"] = with_diff(np.concatenate([_grazing(rng), _under_ball()]))
    parts["non_unit"] = with_diff(_non_unit(rng, N_NON_UNIT))
    parts["differentials"] = _differentials(rng, N_DIFF)
    parts["poles"] = with_diff(_poles(rng))
    total = V * H * W
    n_origins = total - N_INACTIVE - N_SURFACE - sum(len(p) for p in parts.values())
    parts["origins"] = _origins(rng, n_origins)
    # surface starts: the fp32 hit points of the rays so far, fresh directions
    so_far = np.concatenate([parts[k][:, :6] for k in parts]).astype(f32)
    hits, _ = orc.OracleScene(sc).trace_closest(np.concatenate([so_far, np.zeros((len(so_far), 12), f32)], axis=1), threads)
    hp = hits[(hits[:, 0] > 0) & np.isfinite(hits[:, 2:5]).all(axis=1), 2:5]
    pick = rng.integers(len(hp), size=N_SURFACE)
    end = len(parts["critical"]) + len(parts["grazing_normal"])                          # the rays of _under_ball close the class
    under = hits[end - 12:end]
    assert (under[:, 0] > 0).all() and (under[:, 1] < 0.06).all()
    od = _od(hp[pick], _unit(rng, N_SURFACE))
    od[:12, 0:3] = under[:, 2:5]; od[:12, 3:6] = (0.0, 1.0, 0.0)                          # from under the glass ball straight up: a hit 0.02 .. 0.1 away
    parts["on_surface"] = with_diff(od)
    rays = np.zeros((total, 18), f32)
    label = np.full(total, -1, np.int8)
    n = 0
    for k, cls in enumerate(CLASSES):
        p = parts[cls].astype(f32)
        rays[n:n + len(p)] = p; label[n:n + len(p)] = k
        n += len(p)
    assert total - n == N_INACTIVE
    rays[n:, 0:3] = rng.uniform(-3, 3, (N_INACTIVE, 3)); rays[n:, 6:] = rng.uniform(-1, 1, (N_INACTIVE, 12))      # no ray: only the direction says so
    rays[n:, 3:6] = rng.choice(np.array([0.0, -0.0], f32), size=(N_INACTIVE, 3))
    assert np.isfinite(rays[:, :6]).all()
    perm = rng.permutation(total)
    _sets[key] = (sc, np.ascontiguousarray(rays[perm].reshape(V, H, W, 18)), np.ascontiguousarray(label[perm].reshape(V, H, W)))
    return _sets[key]
