"""Mrows/s of the swept-sphere queries (Renderer.query_sweep: rows and answers in device tensors, queued on a torch stream), in the shape
of tools/query_hits_bench.py.

  scene     cfg3 stand-in (host.atrium_scene, 1920x1080, 3 bounces), 2^20 rows per set
  rows      the central 1024 x 1024 pinhole rays of the scene's camera as sweeps with max distance +inf
  order     coherent   8x8-pixel blocks next to each other
            shuffled   the same rows in a seeded random order
            sorted     the shuffled rows with sort=True (RTX_QUERY_SORT): what the library's own sort buys, its cost included
  variants  r1e-3      radius 1e-3 of the scene size, distance only      against  closest   query_closest (distance) on the same rays
            r1e-2      radius 1e-2 of the scene size, distance only
            r1e-2_all  radius 1e-2, all seven channels

Timed with events around `--steps` calls queued back to back on one non-default torch stream (outputs allocated once); the variants
alternate within each of `--rounds` rounds, the medians are reported.  The sorted and the unsorted answers are compared bit for bit first,
and the ball's t against the ray's distance: a ball touches no later than its centre's ray hits.

  python tools/query_sweep_bench.py --out profiles/query_sweep_bench.json
  python tools/query_sweep_bench.py --mask rows      the filtered calls: none (default), ones, half, rows — tools/query_masks.py
"""
import argparse
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(REPO, "cpu-raytracer_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

ORDERS = ("coherent", "shuffled", "sorted")
VARIANTS = ("r1e-3", "closest", "r1e-2", "r1e-2_all")

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
    import pointset
    assert torch.cuda.is_available(), "query_sweep_bench needs a GPU"
    sc = host.atrium_scene(1920, 1080, 3, detail=1)
    lo, hi = pointset.world_box(sc)
    size = float(np.max(hi - lo))
    n = SIDE * SIDE
    r = api.Renderer(sc)
    stream = torch.cuda.Stream()
    mask = query_masks.setup(r, sc, args.mask, n)                        # --mask: the filtered calls (tools/query_masks.py)
    sets, _ = ray_sets(sc)
    rays = {"coherent": torch.from_numpy(sets["coherent"]).cuda(), "shuffled": torch.from_numpy(sets["incoherent"]).cuda()}
    rays["sorted"] = rays["shuffled"]

    def sweeps(t, radius):
        return torch.cat([t, torch.full((n, 1), float("inf"), dtype=torch.float32, device="cuda"), torch.full((n, 1), radius, dtype=torch.float32, device="cuda")], dim=1).contiguous()
    rows = {("r1e-3", k): sweeps(t, 1e-3 * size) for k, t in rays.items()}
    rows.update({("r1e-2", k): sweeps(t, 1e-2 * size) for k, t in rays.items()})
    out = {name: torch.empty((n, k) if k > 1 else (n,), dtype=torch.float32 if dt == np.float32 else torch.int32, device="cuda") for name, (_, dt, k) in api.QUERY_CHANNELS.items()}
    dist = torch.empty((n,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def call(variant, order):
        s = order == "sorted"
        if variant == "closest":
            r.query_closest(rays[order], ("distance",), out={"distance": dist}, sort=s)
        elif variant == "r1e-2_all":
            r.query_sweep(rows[("r1e-2", order)], tuple(api.QUERY_CHANNELS), out=out, sort=s, mask=mask)
        else:
            r.query_sweep(rows[(variant, order)], ("distance",), out={"distance": out["distance"]}, sort=s, mask=mask)

    def timed(variant, order):
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                call(variant, order)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                call(variant, order)
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    # a rate of wrong answers is no rate: sorted == unsorted bit for bit, and a ball is stopped no later than the ray of its centre
    with torch.cuda.stream(stream):
        call("r1e-2_all", "shuffled")
    stream.synchronize()
    plain = {k: t.clone() for k, t in out.items()}
    with torch.cuda.stream(stream):
        call("r1e-2_all", "sorted")
    stream.synchronize()
    for k, t in out.items():
        assert torch.equal(t.view(torch.int32), plain[k].view(torch.int32)), k
    with torch.cuda.stream(stream):
        call("r1e-3", "coherent")
        call("closest", "coherent")
    stream.synchronize()
    later = int((out["distance"] > dist * (1 + 1e-5)).sum())
    answered = int(torch.isfinite(out["distance"]).sum())
    results = []
    for rnd in range(args.rounds):
        for order in ORDERS:
            for variant in VARIANTS:
                ms = timed(variant, order)
                row = {"variant": variant, "order": order, "round": rnd, "rows": n, "ms_per_call": ms, "mrows_per_s": n / ms / 1e3}
                results.append(row)
                print(json.dumps(row), flush=True)
    summary = {}
    for row in results:
        summary.setdefault(f"{row['variant']}/{row['order']}", []).append(row["mrows_per_s"])
    summary = {k: {"median_mrows_per_s": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in summary.items()}
    ratios = {f"{v}_over_closest/{o}": summary[f"{v}/{o}"]["median_mrows_per_s"] / summary[f"closest/{o}"]["median_mrows_per_s"] for o in ORDERS for v in VARIANTS if v != "closest"}
    res = {"tool": "tools/query_sweep_bench.py", "scene": "atrium stand-in 1920x1080", "scene_size": size, "rows_per_call": n, "steps": args.steps, "rounds": args.rounds, "mask": args.mask,
           "rows_answered_r1e-3_coherent": answered, "rows_later_than_the_centre_ray": later, "summary": summary, "ratios": ratios, "rows": results}
    print(json.dumps(summary, indent=1))
    print(json.dumps({"ratios": ratios, "rows_answered_r1e-3_coherent": answered, "rows_later_than_the_centre_ray": later}, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
