"""What the sign costs: Mrows/s of Renderer.query_signed_distance against Renderer.query_nearest on the same rows, and microseconds per
Renderer.blas_pseudonormals step next to Renderer.vertex_normals, in the shape of tools/query_nearest_bench.py.

  scene     cfg3 stand-in (host.atrium_scene, 1920x1080, 3 bounces: one mesh of 255 296 triangles), its soup welded by position into an
            indexed mesh (tools/vertex_normals_bench.py), slot vertices bound, topology set, tables made; 2^20 rows per set
  rows      surface    the hit points of the central 1024 x 1024 pinhole rays moved off the surface along the normal by 1e-3 .. 0.1 (both
                       sides), maximum distance +inf: what a contact probe or a cloth step asks
            uniform    uniform in the scene's box, maximum distance +inf
  order     shuffled   a seeded random order;  sorted: the same rows with sort=True (RTX_QUERY_SORT)
  calls     nearest    query_nearest, distance only
            signed     query_signed_distance, no channel, no feature: one float per row, like `nearest`
            signed+    query_signed_distance with the distance channel and the feature codes
  step      vertex_normals and blas_pseudonormals from rtx_last_kernel_times (HIP events around every launch), per launch, median of --reps

Queries are timed with events around `--steps` calls queued back to back on one non-default torch stream (outputs allocated once); the variants
alternate within each of `--rounds` rounds, the three calls of a group in an order rotated from round to round, and the medians are
reported.  |signed| is compared with query_nearest's distance bit for bit first.

  python tools/query_signed_bench.py --out profiles/query_signed_bench.json
"""
import argparse
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(REPO, "cpu-raytracer_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

SETS = ("surface", "uniform")
ORDERS = ("shuffled", "sorted")
CALLS = ("nearest", "signed", "signed+")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=100, help="calls of the per-step kernels")
    ap.add_argument("--out", help="write the rows and medians as JSON here")
    args = ap.parse_args()

    import numpy as np
    import torch
    from pyrtx import api, host
    from query_bench import ray_sets, SIDE
    assert torch.cuda.is_available(), "query_signed_bench needs a GPU"
    sc = host.atrium_scene(1920, 1080, 3, detail=1)
    assert len(sc.blas) == 1, "the stand-in is one mesh"
    soup = host.atrium_mesh()[0].reshape(-1, 3)
    pos, inv = np.unique(soup, axis=0, return_inverse=True)
    pos, idx = np.ascontiguousarray(pos, np.float32), inv.reshape(-1, 3).astype(np.int32)
    n = SIDE * SIDE
    r = api.Renderer(sc)
    stream = torch.cuda.Stream()
    p_t, i_t = torch.from_numpy(pos).cuda(), torch.from_numpy(idx).cuda()
    nrm_t = torch.empty_like(p_t)
    torch.cuda.synchronize()
    r.bind_blas_vertices(0, host.slot_vertices(sc.blas[0], idx), len(pos))
    r.set_blas_topology(0, i_t, len(pos))
    r.blas_pseudonormals(0, p_t)

    rays = torch.from_numpy(ray_sets(sc)[0]["coherent"]).cuda()
    hit = r.query_closest(rays, ("distance", "position", "normal"))
    rng = np.random.default_rng(2026)
    step = torch.from_numpy((10.0 ** rng.uniform(-3, -1, size=n) * np.where(rng.integers(0, 2, n), 1, -1)).astype(np.float32)).cuda()
    surface = torch.cat([hit["position"] + step[:, None] * hit["normal"], torch.full((n, 1), float("inf"), device="cuda")], dim=1)
    surface[~torch.isfinite(hit["distance"]), 3] = 0.0                   # a ray that missed: no point
    root = sc.tlas_nodes[0]
    uni = rng.uniform(root["aabb_min"].astype(np.float64), root["aabb_max"].astype(np.float64), size=(n, 3)).astype(np.float32)
    perm = torch.from_numpy(rng.permutation(n)).cuda()
    pts = {"surface": surface[perm].contiguous(), "uniform": torch.from_numpy(np.concatenate([uni, np.full((n, 1), np.inf, np.float32)], axis=1)).cuda()}
    dist = torch.empty(n, dtype=torch.float32, device="cuda"); sd = torch.empty_like(dist); ft = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call(name, order, what):
        sort = order == "sorted"
        if what == "nearest":
            r.query_nearest(pts[name], ("distance",), out={"distance": dist}, sort=sort)
        elif what == "signed":
            r.query_signed_distance(pts[name], (), out={"signed_distance": sd}, sort=sort)
        else:
            r.query_signed_distance(pts[name], ("distance",), out={"signed_distance": sd, "feature": ft, "distance": dist}, sort=sort, feature=True)

    def timed(name, order, what):
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                call(name, order, what)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                call(name, order, what)
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    checked = {}
    for name in SETS:                                                    # a rate of wrong answers is no rate
        with torch.cuda.stream(stream):
            call(name, "shuffled", "nearest")
            plain = dist.clone()
            call(name, "sorted", "signed+")
        stream.synchronize()
        assert torch.equal(sd.abs().view(torch.int32), plain.view(torch.int32)) and torch.equal(dist.view(torch.int32), plain.view(torch.int32)), name
        checked[name] = {"answered": int(torch.isfinite(plain).sum()), "negative": int((sd < 0).sum()),
                         "features": {str(k): int(v) for k, v in zip(*[t.tolist() for t in torch.unique(ft, return_counts=True)])}}
    rows = []
    for rnd in range(args.rounds):
        calls = CALLS[rnd % 3:] + CALLS[:rnd % 3]                         # the three calls of a group in a rotated order: no call is always first
        for name, order, what in [(s, o, c) for s in SETS for o in ORDERS for c in calls]:
            ms = timed(name, order, what)
            row = {"set": name, "order": order, "call": what, "round": rnd, "rows": n, "ms_per_call": ms, "mrows_per_s": n / ms / 1e3}
            rows.append(row)
            print(json.dumps(row), flush=True)
    summary = {}
    for row in rows:
        summary.setdefault(f"{row['set']}/{row['order']}/{row['call']}", []).append(row["mrows_per_s"])
    summary = {k: {"median_mrows_per_s": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in summary.items()}
    ratios = {f"{s}/{o}/{c}": summary[f"{s}/{o}/{c}"]["median_mrows_per_s"] / summary[f"{s}/{o}/nearest"]["median_mrows_per_s"] for s in SETS for o in ORDERS for c in CALLS[1:]}

    def step_times(fn):
        for _ in range(5):
            fn()
        r.synchronize(); r.enable_timing(True)
        for _ in range(args.reps):
            fn()
        r.synchronize()
        per = {}
        for name, ms in r.kernel_times():
            per.setdefault(name, []).append(ms)
        r.enable_timing(False)
        kernels = {k: round(float(np.median(v)) * 1e3, 3) for k, v in per.items()}
        return {"kernels_us": kernels, "us": round(sum(kernels.values()), 3)}
    steps = {"triangles": int(len(idx)), "vertices": int(len(pos)), "slots": int(len(sc.blas[0].tri_hot)),
             "vertex_normals": step_times(lambda: r.vertex_normals(0, p_t, nrm_t)), "blas_pseudonormals": step_times(lambda: r.blas_pseudonormals(0, p_t))}
    res = {"tool": "tools/query_signed_bench.py", "scene": "atrium stand-in 1920x1080", "rows_per_call": n, "checked": checked, "steps": args.steps,
           "rounds": args.rounds, "summary": summary, "signed_over_nearest": ratios, "per_step": steps, "rows": rows}
    print(json.dumps(summary, indent=1))
    print(json.dumps({"signed_over_nearest": ratios, "checked": checked, "per_step": steps}, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
