"""The seeded edit sequences of tests/growset.py, checked on the CPU before tests/test_gpu_grow.py spends GPU time on them: the generator is
deterministic per seed, every shadow scene it produces is accepted by the host twins (the balanced BLAS of every new mesh, a valid TLAS, a
frame the oracle renders and rows the twins answer), and the default seeds cover what the sequences are for.  The coverage figures are
conditions, not measurements: where the default seeds miss one, the seeds or the draw weights change, not the condition."""
import numpy as np
import pytest

import growset
import util  # noqa: F401  (the paths)
from test_blas_build_cpu import check_tree
from test_tlas_balanced_cpu import check_tree as check_tlas

f32 = np.float32
SEEDS = growset.default_seeds()
_seq = {}


def seq(seed):
    if seed not in _seq:
        _seq[seed] = growset.sequence(seed)
    return _seq[seed]


def test_the_generator_is_deterministic_per_seed():
    for seed in SEEDS[:3]:
        assert growset.digest(growset.sequence(seed)) == growset.digest(seq(seed)), seed
    assert len({growset.digest(seq(seed)) for seed in SEEDS}) == len(SEEDS), "two seeds give the same sequence"
    assert growset.digest(growset.sequence(0, 4)) == growset.digest(seq(0)[:4]), "a shorter sequence is a prefix"


@pytest.mark.parametrize("seed", SEEDS)
def test_every_shadow_scene_is_legal(seed):
    import orc
    from pyrtx import host
    for k, st in enumerate(seq(seed)):
        sc = st.scene
        what = f"seed {seed} step {k} {st.kind}"
        if st.mesh is not None:                                                  # a BLAS made from a source mesh: the twin's invariants
            blas, sv, order, pos, idx = st.mesh
            check_tree(blas, sv, order, pos, idx)
            assert sc.blas[st.args["id"]] is blas, what
        # every id a kernel would follow is inside its table
        n_mat, n_tex = len(sc.materials), len(sc.textures)
        assert sc.materials["texture_id"].max() < n_tex and sc.instances["blas_id"].max() < len(sc.blas), what
        for b in sc.blas:
            assert 0 <= b.material_offset and b.material_offset + int(b.tri_cold["material_id"].max()) < n_mat, what
        assert all(0 <= m < n_mat for m in list(sc.spheres["material_id"]) + list(sc.planes["material_id"])), what
        for a in (sc.materials["diffuse"], sc.materials["reflection"], sc.sky, sc.instances["world"], sc.spheres["center"]):
            assert np.isfinite(a).all(), what
        assert all(np.isfinite(t.texels).all() for t in sc.textures) and all(np.isfinite(b.tri_hot["position_0"]).all() for b in sc.blas), what
        # the TLAS: balanced over the instances' world boxes as the BLAS roots give them
        if st.kind in ("update_instances", "set_frame") and "positions" in st.args:
            pos, rot = st.args["positions"], st.args["rotations"]
            aabbs = np.zeros((len(pos), 6), f32)
            for i in range(len(pos)):
                root = sc.blas[sc.instances["blas_id"][i]].nodes[0]
                _, mn, mx = host.instance_update(pos[i], rot[i], root["aabb_min"], root["aabb_max"], 0)
                aabbs[i, :3] = mn; aabbs[i, 3:] = mx
            check_tlas(sc.tlas_nodes, sc.tlas_indices, aabbs, True)
        assert len(sc.tlas_indices) == len(sc.instances) and sorted(sc.tlas_indices.tolist()) == list(range(len(sc.instances))), what
        if st.masks is not None:
            assert len(st.masks) == len(sc.instances) + len(sc.spheres) + len(sc.planes), what
        ob = st.observe
        assert ob["kind"] in growset.RENDERS + growset.QUERIES
        if ob["rows"] is not None:
            assert 1 <= len(ob["rows"]) <= growset.ROWS and ob["rows"].dtype == f32 and not np.isnan(ob["rows"]).any(), what
            assert ob["mask"] is None or ob["kind"] in growset.FILTERED, what
    last = seq(seed)[-1].scene
    out = orc.OracleScene(last).render(threads=8)                                # the oracle takes the final frame
    assert out["rgb"].shape == (growset.HEIGHT, growset.WIDTH, 3) and np.isfinite(out["rgb"]).all() and len(np.unique(out["packed"])) > 8, seed
    pts = np.ascontiguousarray(growset.pointset.generate(last, 40, seed)[0][:32])
    assert np.isfinite(host.query_nearest(last, pts, "distance")["distance"]).any(), seed      # and the twins walk it


def test_the_default_seeds_cover_the_growth_kinds():
    steps = [seq(seed) for seed in range(6)]                   # the default seeds, whatever RTX_SEQ_SEEDS says
    cov = growset.coverage(steps)
    for kind in growset.KINDS:                               # every edit occurs at least twice
        assert cov["kinds"][kind] >= 2, (kind, cov["kinds"])
    for kind in growset.RENDERS + growset.QUERIES:           # every entry point is observed
        assert cov["observed"][kind] >= 1, (kind, cov["observed"])
    # a growth of each of the four tables, then (no set_frame in between) a render observation, twice, and a query observation, once
    for table in ("blas", "materials", "textures", "sky"):
        renders, queries = cov["after"][table]
        assert renders >= 2 and queries >= 1, (table, cov["after"])
    assert cov["most_growths"] >= 3, "no sequence grows the same table three times"
    assert cov["mask_ways"] == {"host", "device", "none"}
    drawn = [st.observe for s in steps for st in s]
    assert any(ob["sort"] for ob in drawn) and any(isinstance(ob["mask"], int) for ob in drawn) and any(isinstance(ob["mask"], np.ndarray) for ob in drawn)
    assert any(st.masks is not None and st.observe["mask"] is not None for s in steps for st in s), "no filtered query against a table of object masks"
