"""Mrays/s of the ray queries (Renderer.query_closest / query_occluded: rays and answers in device tensors, queued on a torch stream)
and, beside them, of the same rays through the unit-test hooks rtx_debug_trace_rays / rtx_debug_occluded (host arrays in and out, a
hipMalloc / hipFree and a wait per call): what a caller had before the queries.

  scene     cfg3 stand-in (host.atrium_scene, 1920x1080, 3 bounces); its pinhole rays of the central 1024 x 1024 pixels = 2^20 rays
  order     coherent    8x8-pixel blocks, block after block: every packet of 64 consecutive rays is one block of neighbouring pixels
            incoherent  the same rays in a seeded random order
  rays      primary     those pinhole rays: one origin, directions a pixel apart
            mirror      spread origins: the hit point of each primary ray (query_closest's position channel) moved 1e-3 along the normal, in
                        the mirror direction about the normal; a primary ray that missed keeps a zero direction (no ray), in both orders
  variant   closest_distance   query_closest, distance only (no rebuild)
            closest_all        query_closest, all seven channels
            occluded           query_occluded, every ray as a segment that ends at 1e30
            *_sort             the same three with sort=True (RTX_QUERY_SORT): on the coherent order the cost of the pass itself, on the
                               incoherent order what it buys
            debug_closest      rtx_debug_trace_rays: all 27 RayHit floats back on the host (primary rays only)
            debug_occluded     rtx_debug_occluded

The query variants are timed with events around `--steps` calls queued back to back on one non-default torch stream (outputs allocated
once, so a call allocates nothing); the hooks wait for the device themselves and are timed with the host clock around `--debug-steps`
calls.  One process; the variants alternate within each of `--rounds` rounds, the medians are reported:

  python tools/query_bench.py --out profiles/query_sort_bench.json
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(REPO, "cpu-raytracer_amd"), os.path.join(REPO, "tests")]

SIDE = 1024
ORDERS = ("coherent", "incoherent")
SETS = ("primary", "mirror")
PLAIN_VARIANTS = ("closest_distance", "closest_all", "occluded")
QUERY_VARIANTS = PLAIN_VARIANTS + tuple(v + "_sort" for v in PLAIN_VARIANTS)
DEBUG_VARIANTS = ("debug_closest", "debug_occluded")


def ray_sets(sc):
    """{order: float32 (2^20, 6)} of the central SIDE x SIDE pixels of the scene's camera."""
    import numpy as np
    from pyrtx import api
    full = api.pinhole_rays(sc.camera[0], sc.width, sc.height)[..., :6]
    y0, x0 = (sc.height - SIDE) // 2, (sc.width - SIDE) // 2
    win = full[y0:y0 + SIDE, x0:x0 + SIDE]
    blocks = win.reshape(SIDE // 8, 8, SIDE // 8, 8, 6).transpose(0, 2, 1, 3, 4).reshape(-1, 6)      # (block row, block column, y in block, x in block)
    coherent = np.ascontiguousarray(blocks, np.float32)
    perm = np.random.default_rng(2025).permutation(len(coherent))
    return {"coherent": coherent, "incoherent": np.ascontiguousarray(coherent[perm])}, perm


def mirror_set(r, primary, perm):
    """{order: tensor (2^20, 6)}: the secondary rays of the coherent primary rays (a device tensor), built on the device."""
    import torch
    hit = r.query_closest(primary, ("distance", "position", "normal"))
    d, nrm = primary[:, 3:6], hit["normal"]
    mirrored = d - 2.0 * (d * nrm).sum(dim=1, keepdim=True) * nrm
    rays = torch.cat([hit["position"] + 1e-3 * nrm, mirrored], dim=1)
    rays[~torch.isfinite(hit["distance"])] = 0.0                       # a miss: no ray
    rays = rays.contiguous()
    return {"coherent": rays, "incoherent": rays[torch.from_numpy(perm).cuda()].contiguous()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="queued calls per timed window of a query variant")
    ap.add_argument("--debug-steps", type=int, default=3, help="calls per timed window of a debug hook")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-debug", action="store_true", help="skip the debug hooks")
    ap.add_argument("--out", help="write the rows and medians as JSON here")
    args = ap.parse_args()

    import numpy as np
    import torch
    from pyrtx import api, host
    assert torch.cuda.is_available(), "query_bench needs a GPU"
    sc = host.atrium_scene(1920, 1080, 3, detail=1)
    sets, perm = ray_sets(sc)
    n = SIDE * SIDE
    r = api.Renderer(sc)
    stream = torch.cuda.Stream()
    dev = {("primary", k): torch.from_numpy(v).cuda() for k, v in sets.items()}
    dev.update({("mirror", k): t for k, t in mirror_set(r, dev[("primary", "coherent")], perm).items()})
    seg = {k: torch.cat([t, torch.full((n, 1), 1e30, dtype=torch.float32, device="cuda")], dim=1).contiguous() for k, t in dev.items()}
    host18 = {k: np.concatenate([v, np.zeros((n, 12), np.float32)], axis=1) for k, v in sets.items()}
    host7 = {k: np.concatenate([v, np.full((n, 1), 1e30, np.float32)], axis=1) for k, v in sets.items()}
    out_all = {name: torch.empty((n, k) if k > 1 else (n,), dtype=torch.float32 if dt == np.float32 else torch.int32, device="cuda")
               for name, (_, dt, k) in api.QUERY_CHANNELS.items()}
    out_occ = torch.empty((n,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def query_call(variant, rays, order):
        sort = variant.endswith("_sort")
        base = variant[:-len("_sort")] if sort else variant
        if base == "closest_distance":
            r.query_closest(dev[(rays, order)], ("distance",), out={"distance": out_all["distance"]}, sort=sort)
        elif base == "closest_all":
            r.query_closest(dev[(rays, order)], tuple(api.QUERY_CHANNELS), out=out_all, sort=sort)
        else:
            r.query_occluded(seg[(rays, order)], out=out_occ, sort=sort)

    def time_query(variant, rays, order):
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                query_call(variant, rays, order)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                query_call(variant, rays, order)
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    def time_debug(variant, order):
        call = (lambda: r.debug_trace_rays(host18[order])) if variant == "debug_closest" else (lambda: r.debug_occluded(host7[order]))
        call()
        t0 = time.perf_counter()
        for _ in range(args.debug_steps):
            call()
        return 1e3 * (time.perf_counter() - t0) / args.debug_steps

    rows = []
    for rnd in range(args.rounds):
        for rays in SETS:
            for order in ORDERS:
                for variant in QUERY_VARIANTS + (() if args.no_debug or rays != "primary" else DEBUG_VARIANTS):
                    ms = time_query(variant, rays, order) if variant in QUERY_VARIANTS else time_debug(variant, order)
                    row = {"rays_set": rays, "variant": variant, "order": order, "round": rnd, "rays": n, "ms_per_call": ms, "mrays_per_s": n / ms / 1e3}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    summary = {}
    for rays in SETS:
        for order in ORDERS:
            for variant in QUERY_VARIANTS + DEBUG_VARIANTS:
                v = sorted(x["mrays_per_s"] for x in rows if x["rays_set"] == rays and x["variant"] == variant and x["order"] == order)
                if v:
                    summary[f"{rays}/{variant}/{order}"] = {"median_mrays_per_s": v[len(v) // 2], "min": v[0], "max": v[-1]}
    # what sorting buys or costs: the sorted variant's median rate over the unsorted one's, same rays, same order, same run
    ratios = {}
    for rays in SETS:
        for order in ORDERS:
            for variant in PLAIN_VARIANTS:
                ratios[f"{rays}/{variant}/{order}"] = summary[f"{rays}/{variant}_sort/{order}"]["median_mrays_per_s"] / summary[f"{rays}/{variant}/{order}"]["median_mrays_per_s"]
    # the answers agree: sorted and unsorted bit for bit (every channel, every segment), and on the primary rays with the debug hooks — a
    # rate of wrong answers is no rate
    live = {}
    for rays in SETS:
        for order in ORDERS:
            with torch.cuda.stream(stream):
                query_call("closest_all", rays, order); query_call("occluded", rays, order)
            stream.synchronize()
            plain = {k: t.clone() for k, t in out_all.items()}; plain_occ = out_occ.clone()
            with torch.cuda.stream(stream):
                query_call("closest_all_sort", rays, order); query_call("occluded_sort", rays, order)
            stream.synchronize()
            for k, t in out_all.items():
                assert torch.equal(t.view(torch.int32), plain[k].view(torch.int32)), (rays, order, k)
            assert torch.equal(out_occ, plain_occ), (rays, order)
            live[rays] = int((dev[(rays, order)][:, 3:6] != 0).any(dim=1).sum())
            if not args.no_debug and rays == "primary":
                ref = r.debug_trace_rays(host18[order])
                assert np.array_equal(out_all["distance"].cpu().numpy().view(np.uint32), ref[:, 1].view(np.uint32)), order
                assert np.array_equal(out_occ.cpu().numpy() != 0, r.debug_occluded(host7[order]) != 0), order
    with torch.cuda.stream(stream):
        query_call("closest_all", "primary", "coherent")
    stream.synchronize()
    hits = int(torch.isfinite(out_all["distance"]).sum())
    res = {"tool": "tools/query_bench.py", "scene": "atrium stand-in 1920x1080, central 1024x1024 pinhole rays", "rays": n, "rays_that_hit": hits,
           "live_rays": live,
           "steps": args.steps, "debug_steps": args.debug_steps, "rounds": args.rounds, "summary": summary, "sorted_over_unsorted": ratios, "rows": rows}
    print(json.dumps(summary, indent=1))
    print(json.dumps({"sorted_over_unsorted": ratios}, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
