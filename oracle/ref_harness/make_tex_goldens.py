#!/usr/bin/env python3
"""Reference-pinned texture probes: TEST INFRASTRUCTURE, build container only.

tests/texset.py supplies the synthetic 8-bit textures (every shape of texset.SHAPES8: 1x1 up to 1024x1024, strips, non-square chains and
sides that are no power of two) and, per texture, the labelled adversarial sample set (texset.generate: PER_CLASS rows of each class, those
beyond the oracle's fetch bound dropped).  Each texture is written as a PNG with the repo's own writer (rtxh_image_save_png); the harness
command `texprobe_file <image> <inputs.f32>` makes the reference load it (Texture::load: decode, sRGB -> linear, its own mip chain) and
run Texture::sample on every row.  One run per sampler build of the reference:
    nearest s0_m1_b3_t0, bilinear s0_m1_b3_t1, trilinear s0_m0_b3_t2, aniso s0_m1_b3_t2 (MAX_ANISOTROPY 8), aniso2 s0_m1_b3_t2_a2, ewa s0_m2_b3_t2
Output: tests/golden/unit/texprobe_<build>.npz with, per texture <name>: tile_<name> (32, 32, 2) uint8, which texset.pixels8 expands to the texture's
pixels (the GPU machine needs neither the reference nor the PNG), in_<name> (n, 6), label_<name> (n,) index into `classes`, ref_<name> (n, 3) the reference's colours; `names`.
The archives are written with fixed time stamps: a second run gives the same bytes.

No class had to be left out: every build of the reference terminates on every class, NaN, inf and 2^31 coordinates included (its texel
index goes through Math::mod, its float -> int through cvtss2si, like the oracle's).  The float-texel textures of texset (inf / subnormal
texels, the caller-made 48x48 chain) cannot come from an 8-bit file and stay oracle-only."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402

sys.path.insert(0, os.path.join(mg.REPO, "tests"))
sys.path.insert(0, os.path.join(mg.REPO, "oracle"))
import texset  # noqa: E402
from pyrtx import host  # noqa: E402

BUILDS = {"nearest": "s0_m1_b3_t0", "bilinear": "s0_m1_b3_t1", "trilinear": "s0_m0_b3_t2", "aniso": "s0_m1_b3_t2", "aniso2": "s0_m1_b3_t2_a2",
          "ewa": "s0_m2_b3_t2"}
PER_CLASS, SEED = 28, 20261016


def save_npz(path, arrays):
    """np.savez_compressed with fixed member time stamps."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    if not os.path.isdir(mg.REF):
        sys.exit(f"needs the reference checkout at {mg.REF}")
    mg.stage()
    work = os.path.join(mg.WORK, "texprobe")
    os.makedirs(work, exist_ok=True)
    common = {"classes": np.array(texset.CLASSES), "names": np.array([texset.name8(w, h) for w, h in texset.SHAPES8])}
    lines = ["size 32 32"]
    for w, h in texset.SHAPES8:
        name = texset.name8(w, h)
        px = texset.pixels8(w, h)
        png = os.path.join(work, name + ".png")
        host.save_png(png, texset.pack_rgb(px))
        assert np.array_equal(host.load_image(png)[..., :3], px), name
        in6, labels = texset.generate(texset.texture8(w, h), PER_CLASS, SEED)
        inp = os.path.join(work, name + ".f32")
        np.ascontiguousarray(in6, np.float32).tofile(inp)
        common["tile_" + name] = texset.tile8(w, h); common["in_" + name] = in6; common["label_" + name] = texset.label_index(labels)
        lines.append(f"texprobe_file {png} {inp}")
    d = os.path.join(mg.OUT, "unit")
    for build, variant in BUILDS.items():
        out = mg.run_ref(variant, mg.script_with("cube", lines), "texprobe_" + build)
        arrays = dict(common)
        nan = 0
        for k, name in enumerate(common["names"]):
            io9 = np.fromfile(os.path.join(out, f"texprobe_file{k}.f32"), np.float32).reshape(-1, 9)
            assert np.array_equal(io9[:, :6].view(np.uint32), common["in_" + name].view(np.uint32)), (build, name)
            arrays["ref_" + name] = io9[:, 6:9].copy()
            nan += int(np.isnan(io9[:, 6:9]).any(axis=1).sum())
        path = os.path.join(d, f"texprobe_{build}.npz")
        save_npz(path, arrays)
        print(build, variant, "rows", sum(len(common["in_" + n]) for n in common["names"]), "NaN rows", nan, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
