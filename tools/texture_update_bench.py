"""rtx_update_texture: a launch per mip level against fused passes, and against the only route there was before it.

For textures of 256^2, 1024^2 and 2048^2 float texels and 1024^2 RGBA8 texels that live in a torch tensor:

  (a) microseconds per rtx_update_texture (level 0 converted, whole chain rebuilt) with RTX_TEX_PASS_LEVELS = 1 (one launch per level) and
      = 5 (up to five levels per launch): HIP events around a batch of --batch back-to-back calls on one stream, warm-up discarded, the two
      settings alternating over --rounds rounds in one process; median and [min, max] over the rounds
  (b) the route of before for the same job: tensor.cpu(), host.texture_with_mips (rtxh_texture_mips), rtx_upload_texture, timed end to end
      by the host clock around a synchronise; median of --host-reps

    python tools/texture_update_bench.py [--batch 200] [--rounds 7] [--host-reps 5]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = (("256x256 f32", 256, "f32"), ("1024x1024 f32", 1024, "f32"), ("2048x2048 f32", 2048, "f32"), ("1024x1024 rgba8", 1024, "rgba8"))
SETTINGS = (1, 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=5)
    args = ap.parse_args()
    for p in ("cpu-raytracer_amd", "tests"):
        sys.path.insert(0, os.path.join(REPO, p))
    import numpy as np
    import torch
    import util
    from pyrtx import api, host
    from test_gpu_textures import upload
    if not torch.cuda.is_available():
        print("texture_update_bench: no GPU, nothing measured")
        return 1
    sc, _ = util.load_golden("cube")
    sc.textures = []
    renderers = {}
    callers = os.environ.get("RTX_TEX_PASS_LEVELS")
    for P in SETTINGS:                                   # the knob is read in rtx_create
        os.environ["RTX_TEX_PASS_LEVELS"] = str(P)
        renderers[P] = api.Renderer(sc)
    if callers is None:
        del os.environ["RTX_TEX_PASS_LEVELS"]
    else:
        os.environ["RTX_TEX_PASS_LEVELS"] = callers
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(1)
    rows = []
    with torch.cuda.stream(stream):
        for tid, (name, side, kind) in enumerate(CASES):
            if kind == "f32":
                t = torch.from_numpy(rng.uniform(0, 1, (side, side, 3)).astype(np.float32)).cuda()
            else:
                t = torch.from_numpy(rng.integers(0, 256, (side, side, 4), dtype=np.uint8)).cuda()
            for r in renderers.values():
                r.alloc_texture(tid, side, side, True)
                for _ in range(20):
                    r.update_texture(tid, t)
            stream.synchronize()
            chains = {P: r.read_texture(tid) for P, r in renderers.items()}
            assert util.bit_exact(chains[1].texels, chains[5].texels) and chains[1].desc.tobytes() == chains[5].desc.tobytes()
            us = {P: [] for P in SETTINGS}
            enqueue = {P: [] for P in SETTINGS}          # host time per call of the same loop: where it is the larger one, the host sets the pace
            for _ in range(args.rounds):
                for P in SETTINGS:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream); t0 = time.perf_counter()
                    for _ in range(args.batch):
                        renderers[P].update_texture(tid, t)
                    enqueue[P].append((time.perf_counter() - t0) * 1e6 / args.batch)
                    b.record(stream)
                    b.synchronize()
                    us[P].append(a.elapsed_time(b) * 1e3 / args.batch)
            # the route of before
            r = renderers[1]
            level0 = t if kind == "f32" else None
            ts = []
            for _ in range(args.host_reps):
                stream.synchronize(); t0 = time.perf_counter()
                if kind == "f32":
                    tex = host.texture_with_mips(level0.cpu().numpy())
                else:
                    tex = host.texture_with_mips(host.srgb8_to_linear(t.cpu().numpy()[..., :3]))
                assert upload(r, 8 + tid, tex) == 0
                r.synchronize()
                ts.append((time.perf_counter() - t0) * 1e6)
            assert util.bit_exact(r.read_texture(8 + tid).texels, chains[1].texels)
            level_count = int(chains[1].desc["mip_levels"][0])
            row = {"case": name, "levels": level_count, "texels": int(len(chains[1].texels)),
                   "host_route_us": round(float(np.median(ts)), 1)}
            for P in SETTINGS:
                row[f"P{P}_us"] = round(float(np.median(us[P])), 2)
                row[f"P{P}_min_max_us"] = [round(float(min(us[P])), 2), round(float(max(us[P])), 2)]
                row[f"P{P}_enqueue_us"] = round(float(np.median(enqueue[P])), 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("\n| texture | levels | P = 1, us [min, max] (host enqueue) | P = 5, us [min, max] (host enqueue) | .cpu() + rtxh_texture_mips + rtx_upload_texture, us |")
    print("|---|---|---|---|---|")
    for x in rows:
        print(f"| {x['case']} | {x['levels']} | {x['P1_us']} {x['P1_min_max_us']} ({x['P1_enqueue_us']}) | {x['P5_us']} {x['P5_min_max_us']} ({x['P5_enqueue_us']}) | {x['host_route_us']} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
