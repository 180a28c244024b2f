"""Mrows/s of the swept-box queries (Renderer.query_sweep_box: rows and answers in device tensors, queued on a torch stream), in the shape of
tools/query_sweep_bench.py, beside the two ways there were to ask the question before.

  scene     cfg3 stand-in (host.atrium_scene, 1920x1080, 3 bounces: 255 296 triangles), 2^18 rows per class, seeded
  classes   footprint   flat boxes (0.8 x 0.1 x 1.6 units, a unit = 1 % of the scene's size) hugging the floor at a clearance of 0.2 units,
                        a random yaw, moving horizontally for 10 units
            free        boxes of 1 to 3 units at random orientations in the upper half of the scene's box, any direction, D = +inf
            overlap     the footprint rows with their centres on the floor: they overlap where they start
  variants  box         query_sweep_box, distance only
            box_all     query_sweep_box, all five outputs
            box_sorted  query_sweep_box with sort=True, distance only
            ball        query_sweep with the circumscribed ball |h| on the same rows, distance only: a far larger question for a flat box
            stepped     query_overlapped at --substeps (default 16) places along the path, one launch each, an OR of the flags: it sees
                        nothing thinner than D / substeps (the step is stated in the output)

Timed with events around `--steps` calls queued back to back on one non-default torch stream (outputs allocated once); the variants alternate
within each of `--rounds` rounds, the medians are reported.  Nothing gates on these numbers.  Checked first: sorted == unsorted bit for bit,
the ball never later than the box beyond rounding, and a stepped row that reports an overlap has a box answer within its path.

  python tools/query_sweep_box_bench.py --out profiles/query_sweep_box_bench.json
  python tools/query_sweep_box_bench.py --mask rows      the filtered calls: none (default), ones, half, rows — tools/query_masks.py
"""
import argparse
import json
import os
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [os.path.join(REPO, "cpu-raytracer_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

CLASSES = ("footprint", "free", "overlap")
VARIANTS = ("box", "box_all", "box_sorted", "ball", "stepped")
N = 1 << 18

import query_masks  # noqa: E402


def make_rows(np, lo, hi, size, seed=3):
    rng = np.random.default_rng(seed)
    unit = 0.01 * size
    out = {}
    yaw = rng.uniform(0, 2 * np.pi, N)
    q = np.stack([np.zeros(N), np.sin(yaw / 2), np.zeros(N), np.cos(yaw / 2)], axis=1)
    h = np.tile(np.array([0.4, 0.05, 0.8]) * unit, (N, 1))
    c = np.stack([rng.uniform(lo[0], hi[0], N), np.full(N, lo[1] + h[0, 1] + 0.2 * unit), rng.uniform(lo[2], hi[2], N)], axis=1)
    heading = rng.uniform(0, 2 * np.pi, N)
    d = np.stack([np.cos(heading), np.zeros(N), np.sin(heading)], axis=1)
    D = np.full((N, 1), 10.0 * unit)
    out["footprint"] = np.concatenate([c, d, D, h, q], axis=1).astype(np.float32)
    sunk = c.copy(); sunk[:, 1] = lo[1]
    out["overlap"] = np.concatenate([sunk, d, D, h, q], axis=1).astype(np.float32)
    qf = rng.normal(size=(N, 4)); qf /= np.linalg.norm(qf, axis=1, keepdims=True)
    df = rng.normal(size=(N, 3)); df /= np.linalg.norm(df, axis=1, keepdims=True)
    cf = np.stack([rng.uniform(lo[0], hi[0], N), rng.uniform(0.5 * (lo[1] + hi[1]), hi[1], N), rng.uniform(lo[2], hi[2], N)], axis=1)
    out["free"] = np.concatenate([cf, df, np.full((N, 1), np.inf), rng.uniform(1.0, 3.0, (N, 3)) * unit, qf], axis=1).astype(np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--substeps", type=int, default=16)
    ap.add_argument("--out", help="write the rows and medians as JSON here")
    query_masks.add_argument(ap)
    args = ap.parse_args()

    import numpy as np
    import torch
    from pyrtx import api, host
    import pointset
    assert torch.cuda.is_available(), "query_sweep_box_bench needs a GPU"
    sc = host.atrium_scene(1920, 1080, 3, detail=1)
    lo, hi = pointset.world_box(sc)
    size = float(np.max(hi - lo))
    r = api.Renderer(sc)
    stream = torch.cuda.Stream()
    mask = query_masks.setup(r, sc, args.mask, N)                        # --mask: the filtered calls (tools/query_masks.py)
    host_rows = make_rows(np, lo, hi, size)
    rows = {k: torch.from_numpy(v).cuda() for k, v in host_rows.items()}
    balls = {k: torch.cat([t[:, :7], t[:, 7:10].norm(dim=1, keepdim=True)], dim=1).contiguous() for k, t in rows.items()}
    # the stepped boxes: centre + (j + 1) / substeps * min(D, 10 units) * d, for j < substeps (a free row's path is cut at 10 units: its step is stated)
    reach = {k: torch.clamp(t[:, 6:7], max=0.1 * size) for k, t in rows.items()}
    stepped = {k: [torch.cat([t[:, 0:3] + t[:, 3:6] * reach[k] * ((j + 1) / args.substeps), t[:, 7:14]], dim=1).contiguous() for j in range(args.substeps)] for k, t in rows.items()}
    out = {"distance": torch.empty((N,), device="cuda"), "normal": torch.empty((N, 3), device="cuda"), "object_id": torch.empty((N,), dtype=torch.int32, device="cuda"),
           "triangle_id": torch.empty((N,), dtype=torch.int32, device="cuda"), "axis": torch.empty((N,), dtype=torch.int32, device="cuda")}
    ball_t = torch.empty((N,), device="cuda")
    flag, any_flag = torch.empty((N,), dtype=torch.int32, device="cuda"), torch.zeros((N,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def call(variant, cls):
        if variant == "box":
            r.query_sweep_box(rows[cls], ("distance",), out={"distance": out["distance"]}, mask=mask)
        elif variant == "box_all":
            r.query_sweep_box(rows[cls], tuple(out), out=out, mask=mask)
        elif variant == "box_sorted":
            r.query_sweep_box(rows[cls], ("distance",), out={"distance": out["distance"]}, sort=True, mask=mask)
        elif variant == "ball":
            r.query_sweep(balls[cls], ("distance",), out={"distance": ball_t}, mask=mask)
        else:
            any_flag.zero_()
            for b in stepped[cls]:
                r.query_overlapped(b, out=flag, mask=mask)
                any_flag.bitwise_or_(flag)

    def timed(variant, cls):
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                call(variant, cls)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                call(variant, cls)
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    # a rate of wrong answers is no rate
    checks = {}
    for cls in CLASSES:
        with torch.cuda.stream(stream):
            call("box", cls)
        stream.synchronize()
        plain = out["distance"].clone()
        with torch.cuda.stream(stream):
            call("box_sorted", cls); call("ball", cls); call("stepped", cls)
        stream.synchronize()
        assert torch.equal(out["distance"].view(torch.int32), plain.view(torch.int32)), cls
        dl = rows[cls][:, 3:6].norm(dim=1)
        later = int((ball_t * dl > plain * dl + 1e-4 * size).sum())
        within = torch.isfinite(plain) & (plain * dl <= reach[cls][:, 0] * (1 + 1e-5) + 1e-5 * size)
        unseen = int(((any_flag != 0) & ~within).sum())
        checks[cls] = {"answered": int(torch.isfinite(plain).sum()), "at_t_0": int((plain == 0).sum()), "ball_answered": int(torch.isfinite(ball_t).sum()),
                       "ball_later_than_box": later, "stepped_flags": int((any_flag != 0).sum()), "stepped_flag_without_box_answer": unseen,
                       "box_answer_in_reach_the_steps_missed": int((within & (any_flag == 0)).sum())}
        assert later <= N // 10000 and unseen <= N // 10000, (cls, checks[cls])      # a contact within rounding of a step's place or of the path's end may fall either way
    print(json.dumps(checks, indent=1), flush=True)
    results = []
    for rnd in range(args.rounds):
        for cls in CLASSES:
            for variant in VARIANTS:
                ms = timed(variant, cls)
                row = {"variant": variant, "class": cls, "round": rnd, "rows": N, "ms_per_call": ms, "mrows_per_s": N / ms / 1e3}
                results.append(row)
                print(json.dumps(row), flush=True)
    summary = {}
    for row in results:
        summary.setdefault(f"{row['variant']}/{row['class']}", []).append(row["mrows_per_s"])
    summary = {k: {"median_mrows_per_s": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)} for k, v in summary.items()}
    ratios = {f"box_over_{v}/{c}": summary[f"box/{c}"]["median_mrows_per_s"] / summary[f"{v}/{c}"]["median_mrows_per_s"] for c in CLASSES for v in ("ball", "stepped")}
    res = {"tool": "tools/query_sweep_box_bench.py", "scene": "atrium stand-in 1920x1080", "scene_size": size, "rows_per_call": N, "steps": args.steps, "rounds": args.rounds, "mask": args.mask,
           "substeps": args.substeps, "step_length": 0.1 * size / args.substeps, "checks": checks, "summary": summary, "ratios": ratios, "rows": results}
    print(json.dumps(summary, indent=1))
    print(json.dumps({"ratios": ratios}, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
