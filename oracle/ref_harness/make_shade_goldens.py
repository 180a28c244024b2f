#!/usr/bin/env python3
"""Reference-pinned shade probes: TEST INFRASTRUCTURE, build container only.

tests/shadeset.py supplies small adversarial scenes (exotic indices of refraction, transmittances, reflections and diffuse colours; lights at
and in surfaces, degenerate spot cones, infinite and negative colours, NaN ambient; a mesh with zero, opposed and non-unit normals) as text in
the harness's scene language, and per scene V x H x W labelled primary rays with origins of their own.  The harness command
`shadeprobe <file> <n>` of oracle/_ref/refdump_s0_m1_b3_t2 (lane 1; Raytracer::bounce takes the script's bounce count at run time) sets
Scene::camera.position to each ray's own origin — what rtx_render_rays calls the camera — and runs the ray through the reference's
Raytracer::bounce: colour, distance and the four ray counts of its tree.  The scene the reference traced is compared with the one
pyrtx.assemble builds from the same text (lights, primitives, meshes, instances, and the materials each of them names, by value).
Output: tests/golden/unit/shadeprobe_<scene>.npz: rays (V, H, W, 18), label (V, H, W) index into `classes` (-1: no ray), rgb (V, H, W, 3), dist
(V, H, W), counts (V, H, W, 4) uint16.  CAMERA_SCENE is run a second time with each ray's camera drawn from 16 positions that are no ray's
origin (camera_table (16, 3), camera_index (V, H, W), rgb_cameras): the camera row of orc_shade_rays pinned apart from the origin.
Written with fixed time stamps: a second run gives the same bytes.  Like the other make_*_goldens.py this is run by hand after build()
(which compiles the harness); the tests then check that the committed rays are the generator's.
shadeset.EDITS scenes (lights3) change what the scene language cannot say and stay oracle-only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402
from make_tex_goldens import save_npz  # noqa: E402

sys.path.insert(0, os.path.join(mg.REPO, "tests"))
sys.path.insert(0, os.path.join(mg.REPO, "oracle"))
import shadeset  # noqa: E402
from pyrtx import scene_io as sio  # noqa: E402

SEED = 20261018
CAMERA_SCENE = "lights1"                    # recorded a second time with camera rows of their own


def camera_rows(shape):
    """16 seeded camera positions and which one each ray gets"""
    rng = np.random.default_rng(SEED + 1)
    return rng.uniform((-6, 0, -4), (6, 5, 10), (16, 3)).astype(np.float32), rng.integers(16, size=shape).astype(np.uint8)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def materials_of(sc, ids):
    """the materials `ids` name, by value: the colours, the index of refraction and the texels of the texture"""
    out = []
    for m in np.asarray(sc.materials)[np.asarray(ids, np.int64)]:
        t = int(m["texture_id"])
        out.append((m["diffuse"].tobytes(), m["reflection"].tobytes(), m["transmittance"].tobytes(), m["index_of_refraction"].tobytes(),
                    None if t < 0 else (sc.textures[t].desc.tobytes(), np.asarray(sc.textures[t].texels).tobytes())))
    return out


def main():
    if not os.path.isdir(mg.REF):
        sys.exit(f"needs the reference checkout at {mg.REF}")
    mg.stage()
    data = os.path.join(mg.WORK, "Data")
    for f in ("ShadeNormals.obj", "ShadeNormals.mtl"):                      # the repo's own fixture; a stale BVH cache of it is dropped
        new = open(os.path.join(shadeset.DATA, f), "rb").read()
        dst = os.path.join(data, f)
        if not os.path.exists(dst) or open(dst, "rb").read() != new:
            open(dst, "wb").write(new)
            if os.path.exists(dst + ".bvh"):
                os.remove(dst + ".bvh")
    d = os.path.join(mg.OUT, "unit")
    for name in shadeset.SCRIPTED:
        sc, rays, label = shadeset.generate(name, SEED)
        n = label.size
        inp = os.path.join(mg.WORK, f"shadeprobe_{name}.f32")
        flat = rays.reshape(n, 18)
        np.ascontiguousarray(np.concatenate([flat, flat[:, 0:3]], axis=1), np.float32).tofile(inp)
        script = os.path.join(mg.WORK, f"shade_{name}_gen.txt")
        open(script, "w").write(shadeset.script(name) + f"shadeprobe {inp} {n}\n")
        out = mg.run_ref("s0_m1_b3_t2", script, "shadeprobe_" + name)
        ref_sc = sio.load_scene(os.path.join(out, "scene.rtxs"))
        for what in ("instances", "point_lights", "spot_lights", "dir_lights", "ambient", "tlas_nodes", "tlas_indices"):
            assert same(np.asarray(getattr(sc, what)), np.asarray(getattr(ref_sc, what))), f"{name}: {what} of the assembled scene is not the reference's"
        for what in ("spheres", "planes"):                                  # material ids: the reference's table also holds its base scene's materials
            a, b = getattr(sc, what).copy(), getattr(ref_sc, what).copy()
            assert materials_of(sc, a["material_id"]) == materials_of(ref_sc, b["material_id"]), f"{name}: materials of the {what}"
            a["material_id"] = 0; b["material_id"] = 0
            assert same(a, b), f"{name}: {what} of the assembled scene are not the reference's"
        assert len(sc.blas) == len(ref_sc.blas), name
        for a, b in zip(sc.blas, ref_sc.blas):
            assert same(a.nodes, b.nodes) and same(a.tri_hot, b.tri_hot) and same(a.tri_cold, b.tri_cold), f"{name}: a mesh of the assembled scene is not the reference's"
            local = np.unique(a.tri_cold["material_id"])
            assert materials_of(sc, a.material_offset + local) == materials_of(ref_sc, b.material_offset + local), f"{name}: materials of a mesh"
        io = np.fromfile(os.path.join(out, "shadeprobe.f32"), np.float32).reshape(n, 8)
        extra = {}
        if name == CAMERA_SCENE:                                            # once more with cameras that are not the rays' origins
            table, index = camera_rows(label.shape)
            np.ascontiguousarray(np.concatenate([flat, table[index.reshape(-1)]], axis=1), np.float32).tofile(inp)
            out2 = mg.run_ref("s0_m1_b3_t2", script, "shadeprobe_" + name + "_cameras")
            io2 = np.fromfile(os.path.join(out2, "shadeprobe.f32"), np.float32).reshape(n, 8)
            assert np.array_equal(io2[:, 3:8], io[:, 3:8], equal_nan=True) and not np.array_equal(io2[:, 0:3], io[:, 0:3], equal_nan=True)
            extra = {"camera_table": table, "camera_index": index, "rgb_cameras": io2[:, 0:3].reshape(label.shape + (3,))}
        live = label.reshape(-1) >= 0
        assert (io[live, 4] == 1).all() and not io[~live].any()
        counts = io[:, 4:8]
        assert (counts == np.floor(counts)).all() and counts.max() < 65536
        path = os.path.join(d, f"shadeprobe_{name}.npz")
        save_npz(path, {"classes": np.array(shadeset.CLASSES), "seed": np.int64(SEED), "rays": rays, "label": label,
                        "rgb": io[:, 0:3].reshape(label.shape + (3,)), "dist": io[:, 3].reshape(label.shape),
                        "counts": counts.astype(np.uint16).reshape(label.shape + (4,)), **extra})
        print(name, "rays", int(live.sum()), "counts", counts.sum(axis=0).astype(int).tolist(), "NaN colours", int(np.isnan(io[live, 0:3]).any(axis=1).sum()),
              "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
