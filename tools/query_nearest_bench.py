"""Mpoints/s of the nearest-point queries (Renderer.query_nearest: points and answers in device tensors, queued on a torch stream), in the
shape of tools/query_bench.py.

  scene     cfg3 stand-in (host.atrium_scene, 1920x1080, 3 bounces), 2^20 points per set
  points    surface    the hit points of the central 1024 x 1024 pinhole rays (query_closest's position channel) moved off the surface along
                       the normal by 1e-3 .. 0.1, maximum distance +inf: what a contact probe or a cloth step asks
            radius     uniform in the scene's box, maximum distance 1 (most of them far from any surface: the walk prunes at once)
            infinite   the same points, maximum distance +inf
  order     coherent   neighbours next to each other: 8x8-pixel blocks for `surface`, the Morton order of a 128^3 grid for the uniform sets
            shuffled   the same rows in a seeded random order
            sorted     the shuffled rows with sort=True (RTX_QUERY_SORT): what the library's own Morton sort buys, its cost included
  channels  distance only, and all seven
  scale     query_closest (distance) over the coherent pinhole rays of the same scene

Timed with events around `--steps` calls queued back to back on one non-default torch stream (outputs allocated once); the variants
alternate within each of `--rounds` rounds, the medians are reported.  The sorted and the unsorted answers are compared bit for bit first.

  python tools/query_nearest_bench.py --out profiles/query_nearest_bench.json
  python tools/query_nearest_bench.py --mask rows      the filtered calls: none (default), ones, half, rows — tools/query_masks.py
"""
import argparse
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(REPO, "cpu-raytracer_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

SETS = ("surface", "radius", "infinite")
ORDERS = ("coherent", "shuffled", "sorted")
CHANNELS = ("distance", "all")


def morton_order(p, lo, hi, bits=7):
    import numpy as np
    q = np.clip(((p - lo) / (hi - lo) * (1 << bits)).astype(np.int64), 0, (1 << bits) - 1)
    code = np.zeros(len(p), np.int64)
    for k in range(bits - 1, -1, -1):
        for a in range(3):
            code = (code << 1) | ((q[:, a] >> k) & 1)
    return np.argsort(code, kind="stable")

import query_masks  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", help="write the rows and medians as JSON here")
    query_masks.add_argument(ap)
    args = ap.parse_args()

    import numpy as np
    import torch
    from pyrtx import api, host
    from query_bench import ray_sets, SIDE
    assert torch.cuda.is_available(), "query_nearest_bench needs a GPU"
    sc = host.atrium_scene(1920, 1080, 3, detail=1)
    n = SIDE * SIDE
    r = api.Renderer(sc)
    stream = torch.cuda.Stream()
    mask = query_masks.setup(r, sc, args.mask, n)                        # --mask: the filtered calls (tools/query_masks.py)
    rays = torch.from_numpy(ray_sets(sc)[0]["coherent"]).cuda()
    hit = r.query_closest(rays, ("distance", "position", "normal"))
    rng = np.random.default_rng(2026)
    step = torch.from_numpy((10.0 ** rng.uniform(-3, -1, size=n)).astype(np.float32)).cuda()
    surface = torch.cat([hit["position"] + step[:, None] * hit["normal"], torch.full((n, 1), float("inf"), device="cuda")], dim=1)
    surface[~torch.isfinite(hit["distance"]), 3] = 0.0                   # a ray that missed: no point
    root = sc.tlas_nodes[0]
    lo, hi = root["aabb_min"].astype(np.float64), root["aabb_max"].astype(np.float64)
    uni = rng.uniform(lo, hi, size=(n, 3))
    uni = uni[morton_order(uni, lo, hi)].astype(np.float32)
    perm = torch.from_numpy(rng.permutation(n)).cuda()
    pts = {}
    for name, t in (("surface", surface), ("radius", torch.from_numpy(np.concatenate([uni, np.full((n, 1), 1.0, np.float32)], axis=1)).cuda()),
                    ("infinite", torch.from_numpy(np.concatenate([uni, np.full((n, 1), np.inf, np.float32)], axis=1)).cuda())):
        t = t.contiguous()
        pts[(name, "coherent")] = t
        pts[(name, "shuffled")] = pts[(name, "sorted")] = t[perm].contiguous()
    out_all = {name: torch.empty((n, k) if k > 1 else (n,), dtype=torch.float32 if dt == np.float32 else torch.int32, device="cuda")
               for name, (_, dt, k) in api.QUERY_CHANNELS.items()}
    torch.cuda.synchronize()

    def call(name, order, channels):
        if name == "closest":
            r.query_closest(rays, ("distance",), out={"distance": out_all["distance"]})
        elif channels == "distance":
            r.query_nearest(pts[(name, order)], ("distance",), out={"distance": out_all["distance"]}, sort=order == "sorted", mask=mask)
        else:
            r.query_nearest(pts[(name, order)], tuple(api.QUERY_CHANNELS), out=out_all, sort=order == "sorted", mask=mask)

    def timed(name, order, channels):
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                call(name, order, channels)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                call(name, order, channels)
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    answered = {}
    for name in SETS:                                                    # a rate of wrong answers is no rate: sorted == unsorted, bit for bit
        with torch.cuda.stream(stream):
            call(name, "shuffled", "all")
        stream.synchronize()
        plain = {k: t.clone() for k, t in out_all.items()}
        with torch.cuda.stream(stream):
            call(name, "sorted", "all")
        stream.synchronize()
        for k, t in out_all.items():
            assert torch.equal(t.view(torch.int32), plain[k].view(torch.int32)), (name, k)
        answered[name] = int(torch.isfinite(plain["distance"]).sum())
    rows = []
    for rnd in range(args.rounds):
        for name, order, channels in [(s, o, c) for s in SETS for o in ORDERS for c in CHANNELS] + [("closest", "coherent", "distance")]:
            ms = timed(name, order, channels)
            row = {"set": name, "order": order, "channels": channels, "round": rnd, "rows": n, "ms_per_call": ms, "mrows_per_s": n / ms / 1e3}
            rows.append(row)
            print(json.dumps(row), flush=True)
    summary = {}
    for row in rows:
        summary.setdefault(f"{row['set']}/{row['order']}/{row['channels']}", []).append(row["mrows_per_s"])
    summary = {k: {"median_mrows_per_s": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in summary.items()}
    ratios = {f"{s}/{c}": summary[f"{s}/sorted/{c}"]["median_mrows_per_s"] / summary[f"{s}/shuffled/{c}"]["median_mrows_per_s"] for s in SETS for c in CHANNELS}
    res = {"tool": "tools/query_nearest_bench.py", "scene": "atrium stand-in 1920x1080", "rows_per_call": n, "answered": answered, "steps": args.steps,
           "rounds": args.rounds, "mask": args.mask, "summary": summary, "sorted_over_shuffled": ratios, "rows": rows}
    print(json.dumps(summary, indent=1))
    print(json.dumps({"sorted_over_shuffled": ratios, "answered": answered}, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
