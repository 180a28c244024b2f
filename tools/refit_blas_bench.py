"""rtx_refit_blas against the only route there was before it, for a mesh whose vertices live in device memory.

For a waving cloth (an indexed grid mesh) of roughly 1k, 50k and 255k triangles, one process per size:

  (a) refit     ms per rtx_refit_blas from rtx_last_kernel_times (HIP events around every launch), split per kernel, median of --reps calls;
      rebuild   the route of before: vertices device -> host, rtxh_blas_build, rtx_upload_blas — wall clock around a synchronise, median
  (b) frame     kernel time of one frame (serial launch shape) with the refitted tree against a tree freshly built on the same vertices, at
                three deformation amplitudes (fractions of the cloth's side): a refit keeps the topology of the rest pose, so its boxes
                overlap more the further the mesh moves

    python tools/refit_blas_bench.py [--sizes 1000,50000,255000] [--reps 20] [--width 1280 --height 720]
"""
import argparse
import copy
import json
import os
import subprocess
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
AMPLITUDES = (0.02, 0.1, 0.3)


def cloth(triangles):
    """-> (vertices (V, 3), faces (n, 3)): a grid over [-4, 4]^2 at height 2, lightly rippled so that the rest pose is no single plane"""
    import numpy as np
    side = max(2, int(round((triangles / 2) ** 0.5)))
    g = np.linspace(-4.0, 4.0, side + 1)
    x, z = np.meshgrid(g, g, indexing="xy")
    v = np.stack([x, 2.0 + 0.05 * np.sin(3 * x) * np.cos(2 * z), z + 8.0], -1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(side)[:, None] * (side + 1) + np.arange(side)[None, :]).reshape(-1)
    faces = np.concatenate([np.stack([i, i + 1, i + side + 1], 1), np.stack([i + 1, i + side + 2, i + side + 1], 1)]).astype(np.int32)
    return v, faces


def wave(v, amp, phase=0.0):
    import numpy as np
    out = v.copy()
    out[:, 1] += np.float32(8.0 * amp) * (np.sin(v[:, 0] * 1.3 + phase) * np.cos(v[:, 2] * 0.9)).astype(np.float32)
    return out


def child(args):
    for p in ("cpu-raytracer_amd", "tests"):
        sys.path.insert(0, os.path.join(REPO, p))
    import numpy as np
    import torch
    import util
    from pyrtx import api, host
    verts, faces = cloth(args.triangles)
    n = len(faces)
    up = np.tile(np.array([0, 1, 0], np.float32), (n, 3, 1))
    uv = np.zeros((n, 3, 2), np.float32); mid = np.zeros(n, np.int32)

    sc, _ = util.load_golden("tori16")                             # its plane, lights, sky and materials; one instance of the cloth
    offset = sc.blas[0].material_offset
    sc.config["width"] = args.width; sc.config["height"] = args.height
    sc.camera = host.camera_basis(args.width, args.height, float(np.float32(1.2)), (0.0, 6.0, -1.0), host.axis_angle((1, 0, 0), 0.45))

    def fresh(v):
        return host.build_blas(v[faces], up, uv, mid, offset)

    rest = fresh(verts)
    sc.blas = [rest]
    sc.instances = np.zeros(1, util.sio.INSTANCE)
    pos, rot = np.zeros((1, 3), np.float32), np.array([[0, 0, 0, 1]], np.float32)
    sc.instances, sc.tlas_nodes, sc.tlas_indices = host.scene_update_balanced(sc, pos, rot)
    sv = host.slot_vertices(rest, faces)
    r = api.Renderer(sc)
    r.bind_blas_vertices(0, sv, len(verts))
    p, q = torch.from_numpy(pos).cuda(), torch.from_numpy(rot).cuda()
    out = {"triangles": n, "nodes": len(rest.nodes), "vertices": len(verts)}

    # (a) the refit's kernels
    d = [torch.from_numpy(wave(verts, 0.1, 0.3 * k)).cuda() for k in range(4)]
    for k in range(3):
        r.refit_blas(0, d[k % 4])
    r.synchronize(); r.enable_timing(True)
    for k in range(args.reps):
        r.refit_blas(0, d[k % 4])
    r.synchronize()
    per = {}
    for name, ms in r.kernel_times():
        per.setdefault(name, []).append(ms)
    r.enable_timing(False)
    out["refit_kernels_ms"] = {k: round(float(np.median(v)), 4) for k, v in per.items()}
    out["refit_ms"] = round(sum(out["refit_kernels_ms"].values()), 4)
    t0 = time.perf_counter()                                       # and as the host sees it: calls back to back, one wait at the end
    for k in range(args.reps):
        r.refit_blas(0, d[k % 4])
    r.synchronize()
    out["refit_wall_ms"] = round((time.perf_counter() - t0) * 1e3 / args.reps, 4)
    # the route of before
    ts = {"copy": [], "build": [], "upload": []}
    for k in range(max(3, args.reps // 4)):
        r.synchronize(); t0 = time.perf_counter()
        hv = d[k % 4].cpu().numpy(); t1 = time.perf_counter()
        b = fresh(hv); t2 = time.perf_counter()
        nodes = np.ascontiguousarray(b.nodes); hot = np.ascontiguousarray(b.tri_hot); cold = np.ascontiguousarray(b.tri_cold)
        rc = r.lib.rtx_upload_blas(r.ctx, 0, nodes.ctypes.data, len(nodes), hot.ctypes.data, cold.ctypes.data, len(hot), offset)
        assert rc == 0, rc
        r.synchronize(); t3 = time.perf_counter()
        ts["copy"].append(t1 - t0); ts["build"].append(t2 - t1); ts["upload"].append(t3 - t2)
    out["rebuild_ms"] = {k: round(float(np.median(v)) * 1e3, 3) for k, v in ts.items()}
    out["rebuild_total_ms"] = round(sum(out["rebuild_ms"].values()), 3)

    # (b) the frame: refitted rest-pose tree against a fresh tree on the same vertices
    def frame_ms(rr):
        for _ in range(3):
            rr.render_async(serial=True)
        rr.synchronize(); rr.enable_timing(True)
        for _ in range(5):
            rr.render_async(serial=True)
        rr.synchronize()
        ms = sum(m for _, m in rr.kernel_times()) / 5
        rr.enable_timing(False)
        return ms, rr.framebuffer()[1]

    out["frames"] = []
    for amp in AMPLITUDES:
        v = wave(verts, amp)
        ra = api.Renderer(sc); ra.bind_blas_vertices(0, sv, len(verts))
        dv = torch.from_numpy(v).cuda()
        ra.refit_blas(0, dv); ra.update_instances(p, q)
        ms_refit, img_a = frame_ms(ra)
        sb = copy.copy(sc); sb.blas = [fresh(v)]
        sb.instances, sb.tlas_nodes, sb.tlas_indices = host.scene_update_balanced(sb, pos, rot)
        ms_fresh, img_b = frame_ms(api.Renderer(sb))
        out["frames"].append({"amplitude": amp, "refit_tree_ms": round(ms_refit, 4), "fresh_tree_ms": round(ms_fresh, 4),
                              "differing_pixels": int((img_a != img_b).sum())})
        ra.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,50000,255000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--triangles", type=int, default=1000)
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for t in [int(s) for s in args.sizes.split(",")]:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--triangles", str(t), "--reps", str(args.reps),
                            "--width", str(args.width), "--height", str(args.height)], capture_output=True, text=True, timeout=args.child_timeout)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{t} triangles: failed ({p.returncode})\n{p.stderr[-2000:]}", flush=True)
            return 1
        rows.append(json.loads(line[-1][7:]))
        print(json.dumps(rows[-1]), flush=True)
    print("\n| triangles | refit, ms (kernels) | per kernel | refit, ms (host wall, back to back) | copy + rtxh_blas_build + rtx_upload_blas, ms |")
    print("|---|---|---|---|---|")
    for x in rows:
        per = ", ".join(f"{k} {v}" for k, v in x["refit_kernels_ms"].items())
        rb = x["rebuild_ms"]
        print(f"| {x['triangles']} | {x['refit_ms']} | {per} | {x['refit_wall_ms']} | {x['rebuild_total_ms']} ({rb['copy']} + {rb['build']} + {rb['upload']}) |")
    print("\n| triangles | amplitude | frame with the refitted tree, ms | frame with a fresh tree, ms | differing pixels |")
    print("|---|---|---|---|---|")
    for x in rows:
        for f in x["frames"]:
            print(f"| {x['triangles']} | {f['amplitude']} | {f['refit_tree_ms']} | {f['fresh_tree_ms']} | {f['differing_pixels']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
