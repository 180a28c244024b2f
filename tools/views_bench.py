"""Milliseconds per view of a batch of camera views (rtx_render_views) against the two ways to get N views without it.

  views     one context: rtx_set_views + ONE rtx_render_views call of V views per step (default launch shape)
  serial    one context: V x (rtx_set_frame with the view's camera + rtx_render_tiles of the whole frame) per step (default launch shape)
  contexts  three contexts in flight, the bench.py shape: view v goes to context v % 3, each on its own stream, RTX_RENDER_SERIAL
  views_contexts  both: three contexts in flight, step s = rtx_set_views + ONE rtx_render_views call of V views on context s % 3, RTX_RENDER_SERIAL

Scenes: cfg1 = cube golden (256x256), cfg2 = Monkey golden (1280x720), cfg3 = atrium stand-in (1920x1080, 3 bounces).  The V cameras
are the scene's camera moved sideways in 2 cm steps (a camera path / stereo rig).  Every point runs in a process of its own:

  python tools/views_bench.py --all --out profiles/views_bench.json          # every scene x V in {1, 2, 4, 8, 16} x mode
  python tools/views_bench.py --scene cfg2 --views 8 --mode views            # one point: prints one JSON line
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(REPO, "cpu-raytracer_amd"), os.path.join(REPO, "tests")]

SCENES = ("cfg1", "cfg2", "cfg3")
VIEWS = (1, 2, 4, 8, 16)
MODES = ("views", "serial", "contexts", "views_contexts")


def load_scene(name):
    if name == "cfg3":
        from pyrtx import host
        return host.atrium_scene(1920, 1080, 3, detail=1)
    import util
    sc, _ = util.load_golden({"cfg1": "cube", "cfg2": "monkey"}[name])
    return sc


def cameras(sc, n):
    import numpy as np
    cams = np.repeat(sc.camera[:1], n)
    cams["position"] += np.float32(0.02) * np.arange(n, dtype=np.float32)[:, None] * np.float32([1, 0, 0])
    return cams


def one_point(args):
    import copy
    from pyrtx import api
    sc = load_scene(args.scene)
    cams = cameras(sc, args.views)
    frames = []
    for v in range(args.views):
        f = copy.copy(sc); f.camera = cams[v:v + 1].copy(); frames.append(f)
    if args.mode == "views":
        r = api.Renderer(sc)
        rs = [r]

        def step():
            r.set_views(cams)
            r.render_views_async(0, args.views)
    elif args.mode == "serial":
        r = api.Renderer(sc)
        rs = [r]

        def step():
            for f in frames:
                r.set_frame(f)
                r.render_async()
    elif args.mode == "views_contexts":
        rs = [api.Renderer(sc) for _ in range(3)]
        k = [0]

        def step():
            c = rs[k[0] % 3]; k[0] += 1
            c.set_views(cams)                  # every step, as the other modes upload their cameras every step
            c.render_views_async(0, args.views, serial=True)
    else:
        rs = [api.Renderer(sc) for _ in range(3)]
        k = [0]

        def step():
            for f in frames:
                c = rs[k[0] % 3]; k[0] += 1
                c.set_frame(f)
                c.render_async(serial=True)

    def sync():
        for c in rs:
            c.synchronize()
    steps = args.steps or max(4, 64 // args.views)
    for _ in range(args.warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    dt = time.perf_counter() - t0
    res = {"scene": args.scene, "width": sc.width, "height": sc.height, "views": args.views, "mode": args.mode, "steps": steps,
           "ms_per_step": 1e3 * dt / steps, "ms_per_view": 1e3 * dt / (steps * args.views)}
    for c in rs:
        c.close()
    print(json.dumps(res))


def run_all(args):
    rows = []
    for scene in args.scenes.split(","):
        for v in VIEWS:
            for mode in MODES:
                cmd = [sys.executable, os.path.abspath(__file__), "--scene", scene, "--views", str(v), "--mode", mode, "--warmup", str(args.warmup)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.point_timeout)
                if p.returncode != 0:           # stop at the first failure: no further GPU work after a fault
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    sys.exit(f"views_bench: {scene} V={v} {mode} exited with {p.returncode}")
                row = json.loads(p.stdout.strip().splitlines()[-1])
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/views_bench.py", "rows": rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true", help="every scene x V x mode, one process per point")
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--out", help="--all: write the rows as JSON here")
    ap.add_argument("--point-timeout", type=float, default=300.0)
    ap.add_argument("--scene", choices=SCENES, default="cfg2")
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--mode", choices=MODES, default="views")
    ap.add_argument("--steps", type=int, default=0, help="timed steps (0: max(4, 64 / views))")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    run_all(args) if args.all else one_point(args)


if __name__ == "__main__":
    main()
