"""Ray-level parity of the production traversal kernels (rtx_debug_trace_rays: the closest-hit packet kernel, the per-lane kernel, the
packet kernel with the shared walk at every level; rtx_debug_occluded: the shadow-ray packet and per-lane kernels) on adversarial rays
(tests/rayset.py: box planes, +-0 and subnormal directions, vertices and edges, surface starts, spheres and planes from the inside, far
origins), every RayHit field and the occlusion bit at seven maximum distances, bit for bit:
  * against the REAL reference's records (tests/golden/unit/rayprobe_*.npz, see test_ray_probes.py);
  * against the batch oracle on generated sets over the golden scenes, a chain-shaped BLAS, a TLAS of more than 128 nodes and fuzz scenes;
  * with every schedule knob of both walks (read in rtx_create: one Renderer each), on three of the sets (KNOB_SETS);
  * at batch sizes around a wave and a packet round, and one spanning many rounds."""
import copy
import os

import numpy as np
import pytest

import rayset
import util

pytestmark = pytest.mark.gpu

LANE_TRACE, PACKET_CLOSEST = 16, 64                                 # RTX_RENDER_LANE_TRACE, RTX_RENDER_PACKET_CLOSEST
DATA = os.path.join(util.GOLDEN, "meshes")


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def traceable(sc):
    """The debug hooks need a level-1 ray queue and a light (rtx_debug_trace_rays / rtx_debug_occluded); neither changes what a ray hits."""
    from pyrtx import scene_io as sio
    sc = copy.deepcopy(sc)
    sc.config["bounces"] = max(1, int(sc.config["bounces"][0]))
    if len(sc.point_lights) + len(sc.spot_lights) + len(sc.dir_lights) == 0:
        pl = np.zeros(1, sio.POINT_LIGHT); pl["colour"] = 1.0; pl["position"] = (0.0, 5.0, 0.0)
        sc.point_lights = pl
    return sc


def occluded(r, rays, dist, flags=0):
    """rtx_debug_occluded at k distances per ray: one call over the (n * k) shadow rays."""
    n, k = dist.shape
    od = np.repeat(rays[:, :6], k, axis=0)
    return (r.debug_occluded(np.concatenate([od, dist.reshape(-1, 1)], axis=1), flags) != 0).reshape(n, k)


def check_occ(got, want, labels=None):
    bad = got != want
    if bad.any():
        rows = np.flatnonzero(bad.any(axis=1))
        by = {} if labels is None else {str(c): int((labels[rows] == c).sum()) for c in np.unique(labels[rows])}
        raise AssertionError(f"{len(rows)} rays occlude differently, per distance column {bad.sum(axis=0).tolist()}, by class {by}")


# ---- the reference's own records -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(util.RAY_PROBES))
def test_kernels_reproduce_reference_ray_probes(api, name):
    P = util.load_ray_probe(name)
    sc, _ = util.load_golden(util.RAY_PROBES[name])
    r = api.Renderer(sc)
    rays, ref = P["rays"], P["ref"]
    for flags in (0, LANE_TRACE, PACKET_CLOSEST):
        util.check_hits(r.debug_trace_rays(rays, flags), ref[:, :27], P["label"], P["classes"])
    for flags in (0, LANE_TRACE):
        check_occ(occluded(r, rays, P["dist"], flags), ref[:, 27:] > 0, P["classes"][P["label"]])


# ---- generated sets against the batch oracle -------------------------------------------------------------------------------------------
def chain_blas_scene():
    """cube's materials and lights, one mesh whose BVH is a chain: every inner node = one leaf + the rest (depth 23), triangles in a row."""
    from pyrtx import scene_io as sio
    sc, _ = util.load_golden("cube")
    sc = copy.deepcopy(sc)
    n = 24
    hot = np.zeros(n, sio.TRI_HOT); cold = np.zeros(n, sio.TRI_COLD)
    for i in range(n):
        hot["position_0"][i] = (i * 0.25 - 3.0, -0.6, 0.05 * (i % 5)); hot["position_edge_1"][i] = (0.25, 0.1 * (i % 3), 0.15 * ((i % 2) * 2 - 1)); hot["position_edge_2"][i] = (0.0, 1.2, 0.0)
        cold["normal_0"][i] = (0, 0, -1); cold["material_id"][i] = sc.blas[0].tri_cold["material_id"][0]
    nodes = np.zeros(2 * n, sio.BVH_NODE)
    box = lambda t: np.stack([hot["position_0"][t], hot["position_0"][t] + hot["position_edge_1"][t], hot["position_0"][t] + hot["position_edge_2"][t]])
    inner = [0] + [2 * d + 1 for d in range(1, n - 1)]                # node of chain step d; its children: (leaf d, rest) at (2d + 2, 2d + 3)
    for d in range(n - 1):
        k = inner[d]
        nodes[k]["left_or_first"] = 2 * d + 2; nodes[k]["count"] = np.uint32((1 + d % 3) << 30).astype(np.int32)
        nodes[2 * d + 2]["left_or_first"] = d; nodes[2 * d + 2]["count"] = 1
        b = box(d); nodes[2 * d + 2]["aabb_min"] = b.min(axis=0); nodes[2 * d + 2]["aabb_max"] = b.max(axis=0)
    last = 2 * (n - 2) + 3
    nodes[last]["left_or_first"] = n - 1; nodes[last]["count"] = 1
    b = box(n - 1); nodes[last]["aabb_min"] = b.min(axis=0); nodes[last]["aabb_max"] = b.max(axis=0)
    for d in range(n - 2, -1, -1):                                    # inner boxes bottom-up
        k, l = inner[d], 2 * d + 2
        nodes[k]["aabb_min"] = np.minimum(nodes[l]["aabb_min"], nodes[l + 1]["aabb_min"]); nodes[k]["aabb_max"] = np.maximum(nodes[l]["aabb_max"], nodes[l + 1]["aabb_max"])
    sc.blas[0] = sio.Blas(nodes[:last + 1].copy(), hot, cold, sc.blas[0].material_offset, n)
    sc.tlas_nodes = sc.tlas_nodes.copy()                              # the one instance is unrotated at the origin: its leaf gets the new root box
    sc.tlas_nodes[0]["aabb_min"] = nodes[0]["aabb_min"]; sc.tlas_nodes[0]["aabb_max"] = nodes[0]["aabb_max"]
    return sc


def many_instances_scene():
    """160 instances (a TLAS of more than the 128 nodes whose planes the slab-test split searches, csrc/rtx_trace.h pk_nan_possible_tlas):
    a grid of cubes and tori, half of them unrotated."""
    from pyrtx import assemble
    lines = ["size 64 48", "bounces 1"]
    rng = np.random.default_rng(80)
    for k in range(160):
        x, y, z = (k % 10) * 3.0 - 13.0, (k // 10 % 4) * 3.0 - 4.0, (k // 40) * 3.0 + 6.0
        m = "Cube" if k % 3 else "Torus"
        if k % 2:
            lines.append(f"mesh ./Data/{m}.obj {x} {y} {z}")
        else:
            ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
            lines.append(f"mesh_axis_angle ./Data/{m}.obj {x} {y} {z} {ax[0]:.5f} {ax[1]:.5f} {ax[2]:.5f} {rng.uniform(-3, 3):.4f}")
    lines += ["sphere 0 0 2 0.8", "plane 0 -5 0", "point 20 20 20 0 8 0", "camera 0 0 -10 0 0 0 1"]
    sc = assemble.scene_from_script("\n".join(lines) + "\n", DATA, accel="sbvh")
    assert len(sc.tlas_nodes) > 128, len(sc.tlas_nodes)
    return sc


def fuzz_scene(seed):
    from pyrtx import assemble
    from test_gpu_fuzz import random_scene
    text, mip, tex_mode = random_scene(1000 + seed)
    return assemble.scene_from_script(text, DATA, accel=["sbvh", "bvh", "binned"][seed % 3], mip_filter=mip, texture_mode=tex_mode)


SETS = ["cube", "monkey_small", "materials_aniso", "tori16", "dynamic", "coincident", "chain_blas", "many_instances", "fuzz3", "fuzz7", "fuzz11"]


def load_set(name):
    if name == "chain_blas":
        return chain_blas_scene()
    if name == "many_instances":
        return many_instances_scene()
    if name.startswith("fuzz"):
        return fuzz_scene(int(name[4:]))
    return util.load_golden(name)[0]


_CACHE = {}


def generated(name, n=1024, seed=7):
    """(scene, rays, distances (N, 7), labels, oracle hits, oracle occlusion), cached per module run."""
    key = (name, n, seed)
    if key not in _CACHE:
        import orc
        sc = traceable(load_set(name))
        o = orc.OracleScene(sc)
        rays, dist3, labels, hits = rayset.generate(sc, n, seed, o)
        dist = rayset.all_distances(dist3)
        _CACHE[key] = (sc, rays, dist, labels, hits, o.trace_any(rays, dist))
    return _CACHE[key]


@pytest.mark.parametrize("name", SETS)
def test_generated_rays_equal_the_oracle(api, name):
    sc, rays, dist, labels, hits, occ = generated(name)
    r = api.Renderer(sc)
    classes = np.array(rayset.CLASSES); lab = np.array([list(classes).index(x) for x in labels])
    for flags in (0, LANE_TRACE, PACKET_CLOSEST):
        util.check_hits(r.debug_trace_rays(rays, flags), hits, lab, classes)
    for flags in (0, LANE_TRACE):
        check_occ(occluded(r, rays, dist, flags), occ, labels)


# ---- schedule knobs -------------------------------------------------------------------------------------------------------------------
CLOSEST_KNOBS = [{}, {"RTX_PK_DEFER_CLOSEST": "0"}, {"RTX_PK_DEFER_CLOSEST": "1"}, {"RTX_PK_DEFER_CLOSEST": "4"}, {"RTX_PK_CLOSEST_ASM": "0"},
                 {"RTX_PK_WIDE_CLOSEST": "0"}]
SHADOW_KNOBS = [{}, {"RTX_PK_WIDE": "0"}, {"RTX_PK4_ORDER": "0"}, {"RTX_PK_DEFER": "0"}, {"RTX_PK_DEFER": "64"}, {"RTX_PK_DEFER_LEAF": "0"},
                {"RTX_PK_DEFER_LEAF": "64"}, {"RTX_PK_GROW": "0"}, {"RTX_PK_GROW": "31"}, {"RTX_PK_ORDER": "0"}]
KNOB_SETS = ["materials_aniso", "coincident", "many_instances"]
knob_id = lambda k: "_".join(f"{a[4:].lower()}{b}" for a, b in k.items()) or "default"


@pytest.mark.parametrize("knobs", CLOSEST_KNOBS, ids=knob_id)
@pytest.mark.parametrize("name", KNOB_SETS)
def test_closest_hit_knobs_change_no_ray(api, name, knobs, monkeypatch):
    """The hand-over threshold of the shared walk (RTX_PK_DEFER_CLOSEST 0: every lane private at once; 1, 4: the hand-scheduled shared walk
    for nearly every node), the compiled shared walk and the binary private walk: the packet kernel's rays, with and without
    RTX_RENDER_PACKET_CLOSEST, are the oracle's."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    sc, rays, dist, labels, hits, occ = generated(name)
    r = api.Renderer(sc)
    classes = np.array(rayset.CLASSES); lab = np.array([list(classes).index(x) for x in labels])
    for flags in (0, PACKET_CLOSEST):
        util.check_hits(r.debug_trace_rays(rays, flags), hits, lab, classes)


@pytest.mark.parametrize("knobs", SHADOW_KNOBS, ids=knob_id)
@pytest.mark.parametrize("name", KNOB_SETS)
def test_shadow_knobs_change_no_ray(api, name, knobs, monkeypatch):
    """The shadow-ray walk's schedule knobs at their extremes: the packet kernel's occlusion bits are the oracle's at every distance."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    sc, rays, dist, labels, hits, occ = generated(name)
    r = api.Renderer(sc)
    check_occ(occluded(r, rays, dist), occ, labels)


# ---- batch sizes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_batch_sizes_around_a_wave(api, n):
    """Partial waves and packets, one ray past a packet, one past a queue tile: every ray the oracle's, whatever lands beside it."""
    sc, rays, dist, labels, hits, occ = generated("materials_aniso")
    rng = np.random.default_rng(n)
    pick = rng.permutation(len(rays))[:n] if n <= len(rays) else rng.integers(len(rays), size=n)
    r = api.Renderer(sc)
    for flags in (0, LANE_TRACE, PACKET_CLOSEST):
        util.check_hits(r.debug_trace_rays(rays[pick], flags), hits[pick])
    for flags in (0, LANE_TRACE):
        check_occ(occluded(r, rays[pick], dist[pick], flags), occ[pick])


def test_many_packet_rounds(api):
    """2.4e5 rays (tori16: 16 instances, spheres-free), far more than one round of the persistent packet grid holds: the dynamic fetch
    hands out every packet exactly once and each result lands in its own slot."""
    import orc
    sc = traceable(util.load_golden("tori16")[0])
    o = orc.OracleScene(sc)
    rays = rayset.generate(sc, 2048, 11, o)[0]
    rng = np.random.default_rng(5)
    big = rays[rng.integers(len(rays), size=240_000)].copy()
    big[:, 6:] = rng.uniform(-0.01, 0.01, (len(big), 12)).astype(np.float32)       # every ray distinct in its differentials
    hits, _ = o.trace_closest(big, threads=16)
    r = api.Renderer(sc)
    for flags in (0, PACKET_CLOSEST):
        util.check_hits(r.debug_trace_rays(big, flags), hits)
    d = rayset.shadow_distances(hits[:, 1])[:, 1:2]                                 # exactly at the hit: the tie the strict < decides
    check_occ(occluded(r, big, d), o.trace_any(big, d, threads=16))
