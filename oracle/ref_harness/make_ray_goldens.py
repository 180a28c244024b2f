#!/usr/bin/env python3
"""Reference-pinned ray probes: TEST INFRASTRUCTURE, build container only.

tests/rayset.py draws seeded adversarial rays (box planes, +-0 and subnormal directions, vertices and edges, surface starts, spheres and
planes from the inside, far origins) on a committed golden scene; the harness command `rayprobe <file> <n>` of
oracle/_ref/refdump_s0_m1_b3_t2 runs each through the reference's Scene::trace_primitives (every RayHit field) and
Scene::intersect_primitives at seven maximum distances (t - 1 ulp, t, t + 1 ulp, 0, FLT_MIN, 1e30, inf; t = the closest hit).
The scene the rays were traced against is the committed one (checked byte for byte).
Output: tests/golden/unit/rayprobe_<scene>.npz: rays (n, 18), dist (n, 7), label (n,) index into `classes`, ref (n, 34)."""
import gzip
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402

sys.path.insert(0, os.path.join(mg.REPO, "tests"))
sys.path.insert(0, os.path.join(mg.REPO, "oracle"))
import rayset  # noqa: E402
import util  # noqa: E402

# probe name -> (scene script, script lines the golden was recorded with, golden name in tests/util.py, rays per class, seed)
PROBES = {
    "materials": ("materials", ["size 320 180", "matset mesh:0:0 texture ./Data/LEGOSHLD.tga"], "materials_aniso", 384, 20261016),
    "coincident": ("coincident", [], "coincident", 384, 20261017),
}


def main():
    if not os.path.isdir(mg.REF):
        sys.exit(f"needs the reference checkout at {mg.REF}")
    mg.stage()
    mg.stage_fixture_meshes("coincident")
    d = os.path.join(mg.OUT, "unit")
    for name, (script, extra, golden, n, seed) in PROBES.items():
        sc, _ = util.load_golden(golden)
        rays, dist3, labels, _ = rayset.generate(sc, n, seed)
        dist = rayset.all_distances(dist3)
        inp = os.path.join(mg.WORK, f"rayprobe_{name}.f32")
        np.ascontiguousarray(np.concatenate([rays, dist], axis=1), np.float32).tofile(inp)
        out = mg.run_ref("s0_m1_b3_t2", mg.script_with(script, extra + [f"rayprobe {inp} {len(rays)}"]), "rayprobe_" + name)
        committed = gzip.open(os.path.join(mg.OUT, script, "scene.rtxs.gz"), "rb").read()
        assert committed == open(os.path.join(out, "scene.rtxs"), "rb").read(), f"the probed scene is not the committed {script} scene"
        ref = np.fromfile(os.path.join(out, "rayprobe.f32"), np.float32).reshape(len(rays), 34)
        classes = np.array(rayset.CLASSES)
        label = np.array([list(classes).index(x) for x in labels], np.int8)
        path = os.path.join(d, f"rayprobe_{name}.npz")
        np.savez_compressed(path, rays=rays, dist=dist, label=label, classes=classes, ref=ref)
        print(name, "rays", len(rays), {str(c): int((label == i).sum()) for i, c in enumerate(classes)}, "hits", int((ref[:, 0] > 0).sum()),
              "occluded per distance", ref[:, 27:].sum(axis=0).astype(int).tolist(), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
