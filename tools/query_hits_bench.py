"""Mrows/s of the all-hits segment queries (Renderer.query_hits: segments and answers in device tensors, queued on a torch stream), in the
shape of tools/query_nearest_bench.py.

  scene     cfg3 stand-in (host.atrium_scene, 1920x1080, 3 bounces), 2^20 rows per set
  rows      the central 1024 x 1024 pinhole rays of the scene's camera as segments with max distance +inf
  order     coherent   8x8-pixel blocks next to each other
            shuffled   the same rows in a seeded random order
            sorted     the shuffled rows with sort=True (RTX_QUERY_SORT): what the library's own sort buys, its cost included
  variants  k1         K = 1, distance, no count            against  closest   query_closest (distance) on the same rays
            k4         K = 4, distance, no count
            k4_count   K = 4, distance, with the count
            count      the count-only form                   against  occluded  query_occluded on the same segments
            k4_all     K = 4, all seven channels, with the count

Timed with events around `--steps` calls queued back to back on one non-default torch stream (outputs allocated once); the variants
alternate within each of `--rounds` rounds, the medians are reported.  The sorted and the unsorted answers are compared bit for bit first,
and k1's distance against query_closest's.

  python tools/query_hits_bench.py --out profiles/query_hits_bench.json
  python tools/query_hits_bench.py --mask rows      the filtered calls: none (default), ones, half, rows — tools/query_masks.py
"""
import argparse
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(REPO, "cpu-raytracer_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

ORDERS = ("coherent", "shuffled", "sorted")
VARIANTS = ("k1", "closest", "k4", "k4_count", "count", "occluded", "k4_all")

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
    assert torch.cuda.is_available(), "query_hits_bench needs a GPU"
    sc = host.atrium_scene(1920, 1080, 3, detail=1)
    n = SIDE * SIDE
    r = api.Renderer(sc)
    stream = torch.cuda.Stream()
    mask = query_masks.setup(r, sc, args.mask, n)                        # --mask: the filtered calls (tools/query_masks.py)
    sets, _ = ray_sets(sc)
    rays = {"coherent": torch.from_numpy(sets["coherent"]).cuda(), "shuffled": torch.from_numpy(sets["incoherent"]).cuda()}
    rays["sorted"] = rays["shuffled"]
    seg = {k: torch.cat([t, torch.full((n, 1), float("inf"), dtype=torch.float32, device="cuda")], dim=1).contiguous() for k, t in rays.items()}
    K = 4
    out4 = {name: torch.empty((n, K, k) if k > 1 else (n, K), dtype=torch.float32 if dt == np.float32 else torch.int32, device="cuda")
            for name, (_, dt, k) in api.QUERY_CHANNELS.items()}
    dist1 = torch.empty((n, 1), dtype=torch.float32, device="cuda")
    dist = torch.empty((n,), dtype=torch.float32, device="cuda")
    count = torch.empty((n,), dtype=torch.int32, device="cuda")
    occ = torch.empty((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call(variant, order):
        s = order == "sorted"
        if variant == "k1":
            r.query_hits(seg[order], 1, ("distance",), count=False, out={"distance": dist1}, sort=s, mask=mask)
        elif variant == "closest":
            r.query_closest(rays[order], ("distance",), out={"distance": dist}, sort=s)
        elif variant == "k4":
            r.query_hits(seg[order], K, ("distance",), count=False, out={"distance": out4["distance"]}, sort=s, mask=mask)
        elif variant == "k4_count":
            r.query_hits(seg[order], K, ("distance",), out={"distance": out4["distance"], "count": count}, sort=s, mask=mask)
        elif variant == "count":
            r.query_hits(seg[order], 0, (), out={"count": count}, sort=s, mask=mask)
        elif variant == "occluded":
            r.query_occluded(seg[order], out=occ, sort=s)
        else:
            r.query_hits(seg[order], K, tuple(api.QUERY_CHANNELS), out=dict(out4, count=count), sort=s, mask=mask)

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

    # a rate of wrong answers is no rate: sorted == unsorted bit for bit, and K = 1 without a count is query_closest's distance
    with torch.cuda.stream(stream):
        call("k4_all", "shuffled")
    stream.synchronize()
    plain = {k: t.clone() for k, t in dict(out4, count=count).items()}
    with torch.cuda.stream(stream):
        call("k4_all", "sorted")
        call("k1", "coherent")
        call("closest", "coherent")
    stream.synchronize()
    for k, t in dict(out4, count=count).items():
        assert torch.equal(t.view(torch.int32), plain[k].view(torch.int32)), k
    k1_differs = int((dist1[:, 0].view(torch.int32) != dist.view(torch.int32)).sum())
    hist = torch.bincount(plain["count"].clamp(max=16), minlength=17).tolist()
    rows = []
    for rnd in range(args.rounds):
        for order in ORDERS:
            for variant in VARIANTS:
                ms = timed(variant, order)
                row = {"variant": variant, "order": order, "round": rnd, "rows": n, "ms_per_call": ms, "mrows_per_s": n / ms / 1e3}
                rows.append(row)
                print(json.dumps(row), flush=True)
    summary = {}
    for row in rows:
        summary.setdefault(f"{row['variant']}/{row['order']}", []).append(row["mrows_per_s"])
    summary = {k: {"median_mrows_per_s": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in summary.items()}
    ratios = {f"k1_over_closest/{o}": summary[f"k1/{o}"]["median_mrows_per_s"] / summary[f"closest/{o}"]["median_mrows_per_s"] for o in ORDERS}
    ratios.update({f"count_over_occluded/{o}": summary[f"count/{o}"]["median_mrows_per_s"] / summary[f"occluded/{o}"]["median_mrows_per_s"] for o in ORDERS})
    res = {"tool": "tools/query_hits_bench.py", "scene": "atrium stand-in 1920x1080", "rows_per_call": n, "steps": args.steps, "rounds": args.rounds, "mask": args.mask,
           "count_histogram_to_16": hist, "k1_rows_differing_from_closest": k1_differs, "summary": summary, "ratios": ratios, "rows": rows}
    print(json.dumps(summary, indent=1))
    print(json.dumps({"ratios": ratios, "count_histogram_to_16": hist, "k1_rows_differing_from_closest": k1_differs}, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
