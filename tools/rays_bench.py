"""Milliseconds per frame of ray views (rtx_render_rays of pyrtx.api.pinhole_rays, rays in the context's own buffer) against the camera
views they equal (rtx_render_views of the same cameras), and of the same rays permuted over the whole set (fully incoherent packets).

  source    views = rtx_render_views, rays = rtx_render_rays of the cameras' pinhole rays, permuted = the same rays in a seeded random order
  shape     one      cfg3: one context, one view per call (default launch shape), synchronised every step
            three    cfg3: three contexts in flight, the bench.py shape: step s goes to context s % 3, RTX_RENDER_SERIAL
            views    cfg1: one context, ONE call of 8 views per step (the cube golden, 256x256)

cfg3 = atrium stand-in (1920x1080, 3 bounces), cfg1 = cube golden.  Every point runs in a process of its own, the sources of a shape
alternate within each round so that drift of the clock or of the machine hits them alike; the medians are reported:

  python tools/rays_bench.py --all --out profiles/rays_bench.json
  python tools/rays_bench.py --shape one --source rays            # one point: prints one JSON line
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(REPO, "cpu-raytracer_amd"), os.path.join(REPO, "tests")]

SHAPES = ("one", "three", "views")
SOURCES = ("views", "rays", "permuted")
VIEWS = 8


def one_point(args):
    import numpy as np
    from pyrtx import api
    if args.shape == "views":
        import util
        sc, _ = util.load_golden("cube")
        n = VIEWS
    else:
        from pyrtx import host
        sc = host.atrium_scene(1920, 1080, 3, detail=1)
        n = 1
    cams = np.repeat(sc.camera[:1], n)
    cams["position"] += np.float32(0.02) * np.arange(n, dtype=np.float32)[:, None] * np.float32([1, 0, 0])
    rs = [api.Renderer(sc) for _ in range(3 if args.shape == "three" else 1)]
    if args.source == "views":
        for r in rs:
            r.set_views(cams)
    else:
        rays = np.stack([api.pinhole_rays(c, sc.width, sc.height) for c in cams])
        if args.source == "permuted":
            flat = rays.reshape(-1, rays.shape[-1])
            rays = np.ascontiguousarray(flat[np.random.default_rng(2024).permutation(len(flat))].reshape(rays.shape))
        for r in rs:
            r.set_rays(rays)
    serial = args.shape == "three"

    def step(k):
        r = rs[k % len(rs)]
        if args.source == "views":
            r.render_views_async(0, n, serial=serial)
        else:
            r.render_rays_async(0, n, serial=serial)
        if not serial:
            r.synchronize()

    for k in range(args.warmup):
        step(k)
    for r in rs:
        r.synchronize()
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k)
    for r in rs:
        r.synchronize()
    dt = time.perf_counter() - t0
    res = {"shape": args.shape, "source": args.source, "width": sc.width, "height": sc.height, "views": n, "steps": args.steps,
           "ms_per_step": 1e3 * dt / args.steps}
    res["ms_per_frame"] = res["ms_per_step"] / n
    for r in rs:
        r.close()
    print(json.dumps(res))


def run_all(args):
    rows = []
    for shape in args.shapes.split(","):
        for rnd in range(args.rounds):
            for src in SOURCES:
                cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--source", src, "--steps", str(args.steps), "--warmup", str(args.warmup)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.point_timeout)
                if p.returncode != 0:           # stop at the first failure: no further GPU work after a fault
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    sys.exit(f"rays_bench: {shape} {src} exited with {p.returncode}")
                row = json.loads(p.stdout.strip().splitlines()[-1])
                row["round"] = rnd
                rows.append(row)
                print(json.dumps(row), flush=True)
    summary = {}
    for shape in args.shapes.split(","):
        for src in SOURCES:
            v = sorted(r["ms_per_frame"] for r in rows if r["shape"] == shape and r["source"] == src)
            summary[f"{shape}/{src}"] = {"median_ms_per_frame": v[len(v) // 2], "min": v[0], "max": v[-1]}
    print(json.dumps(summary, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/rays_bench.py", "summary": summary, "rows": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true", help="every shape x source, --rounds alternating rounds, one process per point")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", help="--all: write the rows and medians as JSON here")
    ap.add_argument("--point-timeout", type=float, default=300.0)
    ap.add_argument("--shape", choices=SHAPES, default="one")
    ap.add_argument("--source", choices=SOURCES, default="rays")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    run_all(args) if args.all else one_point(args)


if __name__ == "__main__":
    main()
