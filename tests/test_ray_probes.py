"""Reference-pinned ray probes (tests/golden/unit/rayprobe_*.npz, made by oracle/ref_harness/make_ray_goldens.py from tests/rayset.py's
adversarial classes): every RayHit field of the REAL reference's Scene::trace_primitives and its Scene::intersect_primitives at seven
maximum distances (the closest hit t - 1 ulp, t, t + 1 ulp, 0, FLT_MIN, 1e30, inf), on `materials` and on the coincident-geometry scene.
CPU: the oracle's batch entry points reproduce them bit for bit.  The GPU side is tests/test_gpu_rays.py."""
import os

import numpy as np
import pytest

import util

@pytest.mark.parametrize("name", list(util.RAY_PROBES))
def test_oracle_reproduces_reference_ray_probes(name):
    import orc
    P = util.load_ray_probe(name)
    sc, _ = util.load_golden(util.RAY_PROBES[name])
    o = orc.OracleScene(sc)
    hits, ids = o.trace_closest(P["rays"])
    util.check_hits(hits, P["ref"][:, :27], P["label"], P["classes"])
    occ = o.trace_any(P["rays"], P["dist"])
    assert np.array_equal(occ, P["ref"][:, 27:] > 0), np.argwhere(occ != (P["ref"][:, 27:] > 0))[:8].tolist()
    # the ids name the primitive whose fields were returned: material ids agree, misses have none
    hit = P["ref"][:, 0] > 0
    assert np.array_equal(ids[:, 0], np.where(hit, P["ref"][:, 8].astype(np.int32), -1))
    assert np.array_equal(ids[:, 1] >= 0, hit) and np.array_equal(ids[~hit], np.full((int((~hit).sum()), 3), -1))


@pytest.mark.parametrize("name", list(util.RAY_PROBES))
def test_ray_probes_cover_every_class_and_edge(name):
    """Guards against a vacuous probe set: every class present, exact ties of the shadow distance resolved both ways, ties in the walk."""
    P = util.load_ray_probe(name)
    assert set(np.unique(P["label"]).tolist()) == set(range(len(P["classes"])))
    ref, dist = P["ref"], P["dist"]
    hit = ref[:, 0] > 0
    assert np.array_equal(dist[hit, 1], ref[hit, 1])                              # column 1 is the closest-hit distance itself
    assert (ref[:, 30] == 0).all() and (ref[:, 31] == 0).all()                    # max distance 0 and FLT_MIN: nothing lies that close
    assert int((ref[hit, 29] > ref[hit, 28]).sum()) > len(ref) // 4               # the hit itself occludes at t + 1 ulp and not at t
    d = P["rays"][:, 3:6]
    assert ((d == 0) & np.signbit(d)).any() and ((d != 0) & (np.abs(d) < np.finfo(np.float32).tiny)).any()   # -0.0 and subnormal directions
