"""rtx_set_blas_topology / rtx_blas_vertex_normals against the route there was before them, for a mesh whose vertices live in device memory.

Two meshes of about 255k triangles, one process each:

  atrium   the cfg3 stand-in mesh (host.atrium_mesh), its triangle soup welded by position into an indexed mesh: valence as a scene has it
  sphere   a UV sphere of 1024 segments and 126 rings: two poles of valence 1024 among vertices of valence 6 — the list one lane walks alone

For each:
  topology  ms per rtx_set_blas_topology (keys, radix sort, offsets) from rtx_last_kernel_times (HIP events around every launch), split per
            launch, median of --reps calls, and the host's wall time per call (calls back to back, one wait at the end)
  normals   the same for rtx_blas_vertex_normals (face vectors, sum per vertex)
  torch     the route of before on the same tensors: cross, index_add_ (float atomics: not reproducible), normalize — torch events around
            --reps calls after a warm-up, per call
and, as a check, that the device normals equal host.vertex_normals bit for bit and how far the torch route is from them.

    python tools/vertex_normals_bench.py [--meshes atrium,sphere] [--reps 200]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def uv_sphere(segments=1024, rings=126):
    """-> (positions (V, 3) f32, indices (T, 3) i32): V = segments * (rings - 1) + 2, T = 2 * segments * (rings - 1)"""
    import numpy as np
    lat = np.pi * np.arange(1, rings) / rings
    lon = 2 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.repeat(np.cos(lat)[:, None], segments, 1), np.outer(np.sin(lat), np.sin(lon))], -1)
    pos = np.concatenate([[[0, 1, 0]], ring.reshape(-1, 3), [[0, -1, 0]]]).astype(np.float32)
    j = np.arange(segments); jn = (j + 1) % segments
    tris = [np.stack([np.zeros(segments, np.int64), 1 + jn, 1 + j], 1)]
    for i in range(rings - 2):
        a, b = 1 + i * segments, 1 + (i + 1) * segments
        tris += [np.stack([a + j, a + jn, b + j], 1), np.stack([a + jn, b + jn, b + j], 1)]
    last = 1 + (rings - 2) * segments
    tris.append(np.stack([np.full(segments, len(pos) - 1), last + j, last + jn], 1))
    return pos, np.concatenate(tris).astype(np.int32)


def welded_atrium():
    import numpy as np
    from pyrtx import host
    soup = host.atrium_mesh()[0].reshape(-1, 3)
    pos, inv = np.unique(soup, axis=0, return_inverse=True)
    return np.ascontiguousarray(pos, np.float32), inv.reshape(-1, 3).astype(np.int32)


def child(args):
    for p in ("cpu-raytracer_amd", "tests"):
        sys.path.insert(0, os.path.join(REPO, p))
    import numpy as np
    import torch
    import util
    from pyrtx import api, host
    pos, idx = welded_atrium() if args.mesh == "atrium" else uv_sphere()
    T, V = len(idx), len(pos)
    valence = np.bincount(idx.reshape(-1), minlength=V)
    out = {"mesh": args.mesh, "triangles": T, "vertices": V, "valence_median": int(np.median(valence)), "valence_max": int(valence.max())}
    sc, _ = util.load_golden("cube")                               # any uploaded BLAS will do: the topology's counts are its own
    r = api.Renderer(sc)
    p, i = torch.from_numpy(pos).cuda(), torch.from_numpy(idx).cuda()
    n = torch.empty_like(p)
    torch.cuda.synchronize()

    def timed(call):
        for _ in range(5):
            call()
        r.synchronize(); r.enable_timing(True)
        for _ in range(args.reps):
            call()
        r.synchronize()
        per = {}
        for name, ms in r.kernel_times():
            per.setdefault(name, []).append(ms)
        r.enable_timing(False)
        kernels = {k: round(float(np.median(v)), 5) for k, v in per.items()}
        t0 = time.perf_counter()
        for _ in range(args.reps):
            call()
        r.synchronize()
        return {"kernels_ms": kernels, "ms": round(sum(kernels.values()), 5), "wall_ms": round((time.perf_counter() - t0) * 1e3 / args.reps, 5)}

    r.set_blas_topology(0, i, V)                                    # the alloc
    out["topology"] = timed(lambda: r.set_blas_topology(0, i, V))
    out["normals"] = timed(lambda: r.vertex_normals(0, p, n))
    r.synchronize()
    got = n.cpu().numpy()
    out["equals_host_twin"] = bool(got.tobytes() == host.vertex_normals(pos, idx).tobytes())

    il = i.long()
    flat = il.reshape(-1)

    def torch_route():
        tri = p[il]
        f = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
        acc = torch.zeros_like(p)
        acc.index_add_(0, flat, f.repeat_interleave(3, 0))
        return torch.nn.functional.normalize(acc, dim=1)

    for _ in range(5):
        ref = torch_route()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        ref = torch_route()
    b.record(); torch.cuda.synchronize()
    out["torch_ms"] = round(a.elapsed_time(b) / args.reps, 5)
    again = torch_route(); torch.cuda.synchronize()
    out["torch_reproducible"] = bool(torch.equal(ref, again))
    out["torch_max_abs_difference"] = float((ref.cpu().numpy().astype(np.float64) - got).__abs__().max())
    out["normals_over_torch"] = round(out["normals"]["ms"] / out["torch_ms"], 4)
    r.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="atrium,sphere")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--mesh", default="atrium")
    args = ap.parse_args()
    if args.child:
        return child(args)
    rows = []
    for m in args.meshes.split(","):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--mesh", m, "--reps", str(args.reps)],
                           capture_output=True, text=True, timeout=args.child_timeout)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{m}: failed ({p.returncode})\n{p.stderr[-2000:]}", flush=True)
            return 1
        rows.append(json.loads(line[-1][7:]))
        print(json.dumps(rows[-1]), flush=True)
    if len(rows) == 2:
        print(json.dumps({"sphere_over_atrium_normals": round(rows[1]["normals"]["ms"] / rows[0]["normals"]["ms"], 4),
                          "sphere_over_atrium_per_triangle": round(rows[1]["normals"]["ms"] / rows[1]["triangles"] / (rows[0]["normals"]["ms"] / rows[0]["triangles"]), 4)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
