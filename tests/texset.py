"""Synthetic textures and seeded adversarial sample sets for the texture and sky samplers (plain numpy; the oracle supplies each sample's
texel-fetch count, which bounds what a lane of the device's debug kernel has to walk).

Textures (scene_io.Texture: desc + texels), by name in SHAPES8 / FLOAT_TEXTURES:
  8-bit ones    "<w>x<h>": pixels8(w, h) decoded like Texture::load (sRGB byte -> linear float), box-filter chain from
                host.texture_with_mips where both sides are powers of two (Texture.cpp:49-55), one level otherwise.  These are the
                textures the reference can load from a PNG, so they carry the reference-pinned probes (tests/golden/unit/texprobe_*.npz).
  float ones    "32x32_special" random float texels with exact 0, 1, subnormal, 1e30 and inf among them; "48x48_chain" a caller-made
                chain on a base that is no power of two (48, 24, 12, 6, 3, 1: six levels, mipmapped = 1), which the ABI accepts and
                the reference never builds.  Oracle-only.
Mip-mapped shapes have an aspect ratio of at most 4:1 (an EWA footprint is sized by the width alone); strips have one level.

samples(tex, n, seed) -> (in6 (N, 6) float32: s, t, ds_dx, ds_dy, dt_dx, dt_dy; labels (N,) class names), n rows per class of CLASSES:
  uniform        s, t in [-2, 2), derivatives of random sign scaled by 2^-10 .. 1 (the distribution of the reference harness's probes)
  texel_centre   (k + 0.5) / extent: s * w - 0.5 an integer, the cvtss2si tie of the bilinear footprint
  texel_corner   k / extent, 0 and +-1 exactly among them
  neg_wrap       negative coordinates down to -1e6
  far            |s| of 1e6, 2^24, and just below / above 2^31 / extent (where float -> int turns into the integer indefinite)
  special_st     +-0, +-1e-30, +-inf, NaN, +-1e38 in either or both coordinates
  zero_deriv     all four derivatives zero (what the shade kernel passes without ray differentials)
  axis_zero      one or two of the four derivatives zero
  lod_boundary   power-of-two footprints, 2^(-j - 0.5), and their neighbours up to 2 ulp away: lod and lod - 0.5 on and beside integers
                 for the LOD formula of each of the three mip filters
  tap_counts     ext_long / ext_short exactly 1 .. 17 and one ulp either side: every anisotropic tap count, odd tails, the clamp
  eccentric      ratios of 1e3 .. 1e6 (EWA's eccentricity clamp) and major axes of exactly the texture's width or height, one ulp either
                 side, and between the two (8x2 and 2x8 are small enough for that to change the level)
  minor_tiny     minor axes around 1e-5 (EWA's hand-over to the bilinear filter)
  special_deriv  +-inf, NaN, +-1e38, 1e-30, -0.0 among the derivatives

generate(tex, n, seed) -> (in6, labels) keeps the samples that cost at most MAX_FETCHES oracle texel fetches under every configuration of
CONFIGS and asserts that fewer than 1 % of any class were dropped: a cost condition, not a tolerance.
"""
import numpy as np

f32 = np.float32
MAX_FETCHES = 65536
CLASSES = ("uniform", "texel_centre", "texel_corner", "neg_wrap", "far", "special_st", "zero_deriv", "axis_zero", "lod_boundary",
           "tap_counts", "eccentric", "minor_tiny", "special_deriv")
# name -> (texture_mode, mip_filter, max_anisotropy): RTX_TEXTURE_NEAREST / BILINEAR / MIPMAP, RTX_MIP_TRILINEAR / ANISOTROPIC / EWA
CONFIGS = {"nearest": (0, 1, 8.0), "bilinear": (1, 1, 8.0), "trilinear": (2, 0, 8.0), "aniso1": (2, 1, 1.0), "aniso2": (2, 1, 2.0),
           "aniso8": (2, 1, 8.0), "aniso16": (2, 1, 16.0), "ewa8": (2, 2, 8.0), "ewa16": (2, 2, 16.0)}
SHAPES8 = [(1, 1), (2, 2), (256, 1), (1, 64), (64, 16), (16, 64), (32, 32), (1024, 1024), (300, 200), (501, 1), (3, 5), (8, 2), (2, 8)]
FLOAT_TEXTURES = ["32x32_special", "48x48_chain"]


def name8(w, h):
    return f"{w}x{h}"


def tile8(w, h, seed=20261016):
    """The seeded (32, 32, 2) uint8 tile a texture's red and green channels repeat (what the stored fixtures keep of a texture)."""
    return np.random.default_rng([seed, w, h]).integers(0, 256, (32, 32, 2), dtype=np.uint8)


def pixels8(w, h, tile=None):
    """(h, w, 3) uint8.  Red and green repeat a 32x32 tile (so that a fixture need not store a megapixel), green XORed with the tile's
    position; blue is the tile's own number, so that a wrap that is off by whole tiles still shows."""
    tile = tile8(w, h) if tile is None else tile
    y, x = np.mgrid[0:h, 0:w]
    out = np.zeros((h, w, 3), np.uint8)
    out[..., 0] = tile[y % 32, x % 32, 0]
    out[..., 1] = tile[y % 32, x % 32, 1] ^ ((x // 32) * 7 + (y // 32) * 13).astype(np.uint8)
    out[..., 2] = ((x // 32) + 37 * (y // 32) + 11).astype(np.uint8)
    return out


def pack_rgb(px):
    """(h, w, 3) uint8 -> (h, w) uint32 0x00RRGGBB (host.save_png's input)."""
    p = px.astype(np.uint32)
    return (p[..., 0] << 16) | (p[..., 1] << 8) | p[..., 2]


def numpy_chain(level0):
    """Texture::load's chain (Texture.cpp:76-117) restated independently of the host library: (h, w, 3) float32 -> (mip_levels, offsets,
    texels (n, 3)); one level unless both sides are powers of two."""
    h, w, _ = level0.shape
    levels = [np.asarray(level0, f32)]
    if w & (w - 1) == 0 and h & (h - 1) == 0:
        n = 1 + int(np.log2(f32(min(w, h))))
        while levels[-1].shape[0] >= 2 and levels[-1].shape[1] >= 2:
            p = levels[-1]
            with np.errstate(all="ignore"):
                levels.append((((p[0::2, 0::2] + p[0::2, 1::2]) + p[1::2, 0::2]) + p[1::2, 1::2]) * f32(0.25))
        assert len(levels) == n, (w, h, len(levels), n)
    offsets = np.cumsum([0] + [l.shape[0] * l.shape[1] for l in levels[:-1]]).tolist()
    return len(levels), offsets, np.concatenate([l.reshape(-1, 3) for l in levels]).astype(f32)


def _texture(w, h, mipmapped, offsets, texels):
    from pyrtx import scene_io as sio
    d = np.zeros(1, sio.TEXTURE_DESC)
    d["width"] = w; d["height"] = h; d["mipmapped"] = mipmapped; d["mip_levels"] = len(offsets)
    d["mip_offsets"][0, :len(offsets)] = offsets
    return sio.Texture(d, np.ascontiguousarray(texels, f32))


def texture_from_level0(level0):
    """The chain the host library builds (rtxh_texture_mips) for power-of-two shapes, one level otherwise."""
    from pyrtx import host
    h, w, _ = level0.shape
    if w & (w - 1) == 0 and h & (h - 1) == 0:
        return host.texture_with_mips(np.ascontiguousarray(level0, f32))
    return _texture(w, h, 0, [0], np.asarray(level0, f32).reshape(-1, 3))


def texture8(w, h, tile=None):
    from pyrtx import host
    return texture_from_level0(host.srgb8_to_linear(pixels8(w, h, tile)))


def float_texture(name, seed=5):
    rng = np.random.default_rng([seed, len(name)])
    if name == "32x32_special":
        t = rng.uniform(0, 1, (32, 32, 3)).astype(f32)
        special = np.array([0.0, 1.0, 1e-45, 1e-39, 1e30, np.inf], f32)
        k = rng.integers(0, 32 * 32 * 3, 96)
        t.reshape(-1)[k] = special[rng.integers(len(special), size=len(k))]
        with np.errstate(all="ignore"):
            return texture_from_level0(t)
    if name == "48x48_chain":
        sizes = [48, 24, 12, 6, 3, 1]
        offsets = np.cumsum([0] + [s * s for s in sizes[:-1]]).tolist()
        return _texture(48, 48, 1, offsets, rng.uniform(0, 1, (sum(s * s for s in sizes), 3)).astype(f32))
    raise KeyError(name)


def all_textures():
    """name -> Texture: every 8-bit shape, then the float ones."""
    out = {name8(w, h): texture8(w, h) for w, h in SHAPES8}
    out.update({n: float_texture(n) for n in FLOAT_TEXTURES})
    return out


def unmipped(tex):
    """The same level 0 as a build of the reference without TEXTURE_SAMPLE_MODE_MIPMAP holds it: no chain (Texture.cpp:49-55)."""
    w, h = int(tex.desc["width"][0]), int(tex.desc["height"][0])
    return _texture(w, h, 0, [0], tex.texels[:w * h])


# ---- sample classes --------------------------------------------------------------------------------------------------------------------
def _ulps(x, k):
    """x moved by k ulps (k an int array), sign-magnitude order; x finite and non-zero."""
    x = np.asarray(x, f32)
    return (x.view(np.int32) + np.asarray(k, np.int32)).view(f32)


def _uniform_derivs(rng, n):
    scale = np.exp2(-10.0 * rng.random(n))
    d = (rng.random((n, 4)) - 0.5) * scale[:, None]
    d[:, 1] *= np.where(rng.random(n) < 0.3, 0.05, 1.0)
    d[:, 3] *= np.where(rng.random(n) < 0.3, 0.05, 1.0)
    return d.astype(f32)                                                       # columns: ds_dx, ds_dy, dt_dx, dt_dy


def _st(rng, n):
    return rng.uniform(-2, 2, (n, 2)).astype(f32)


def _axes(rng, n, long_, short_):
    """Derivatives whose screen-space extents are (long_, short_) exactly: the long one along x or y, carried by s or by t, random signs;
    the partner on each axis is smaller."""
    d = np.zeros((n, 4), f32)
    long_ = np.asarray(long_, f32); short_ = np.asarray(short_, f32)
    for i in range(n):
        x_major, on_s = rng.random() < 0.5, rng.random() < 0.5
        small = f32(rng.uniform(0, 0.9))
        big = (long_[i], f32(long_[i] * small)) if on_s else (f32(long_[i] * small), long_[i])         # (ds, dt) of the long axis
        lit = (short_[i], f32(short_[i] * small)) if rng.random() < 0.5 else (f32(short_[i] * small), short_[i])
        (d[i, 0], d[i, 2]), (d[i, 1], d[i, 3]) = (big, lit) if x_major else (lit, big)
    return d * rng.choice(np.array([-1.0, 1.0], f32), (n, 4))


def samples(tex, n=64, seed=0):
    w, h = int(tex.desc["width"][0]), int(tex.desc["height"][0])
    levels = max(int(tex.desc["mip_levels"][0]), 1 + int(np.log2(min(w, h))))
    rng = np.random.default_rng([seed, w, h])
    wh = np.array([w, h], f32)
    parts = {}

    def put(name, st, d):
        parts[name] = np.concatenate([np.asarray(st, f32), np.asarray(d, f32)], axis=1)

    put("uniform", _st(rng, n), _uniform_derivs(rng, n))

    k = rng.integers(-2 * wh.astype(int), 2 * wh.astype(int) + 1, (n, 2))
    st = ((k + 0.5).astype(f32) / wh).astype(f32)
    one = rng.random(n) < 0.25                                                 # a quarter: only one axis on a centre
    st[one, rng.integers(0, 2, int(one.sum()))] = _st(rng, int(one.sum()))[:, 0]
    put("texel_centre", st, _uniform_derivs(rng, n))

    k = rng.integers(-2 * wh.astype(int), 2 * wh.astype(int) + 1, (n, 2))
    st = (k.astype(f32) / wh).astype(f32)
    st[:6] = np.array([[0, 0], [1, 1], [-1, -1], [0, 1], [-1, 0], [1, -1]], f32)[:min(6, n)]
    put("texel_corner", st, _uniform_derivs(rng, n))

    put("neg_wrap", -np.exp(rng.uniform(np.log(1e-3), np.log(1e6), (n, 2))), _uniform_derivs(rng, n))

    edge = (f32(2.0) ** 31 / wh).astype(f32)                                   # s * extent == 2^31 (extents that are powers of two: exactly)
    far = np.zeros((n, 2), f32)
    for i in range(n):
        for a in range(2):
            c = int(rng.integers(5))
            v = [f32(1e6), f32(2.0 ** 24), _ulps(edge[a], -int(rng.integers(1, 5))), _ulps(edge[a], int(rng.integers(0, 5))),
                 f32(rng.uniform(-2, 2))][c]
            far[i, a] = v * (1 if rng.random() < 0.5 or c == 4 else -1)
    put("far", far, _uniform_derivs(rng, n))

    sp = np.array([0.0, -0.0, 1e-30, -1e-30, np.inf, -np.inf, np.nan, 1e38, -1e38], f32)
    st = _st(rng, n)
    which = rng.integers(0, 3, n)                                              # s, t or both
    pick = sp[rng.integers(len(sp), size=(n, 2))]
    st[which != 1, 0] = pick[which != 1, 0]; st[which != 0, 1] = pick[which != 0, 1]
    put("special_st", st, _uniform_derivs(rng, n))

    put("zero_deriv", _st(rng, n), np.where(rng.random((n, 4)) < 0.5, f32(0.0), f32(-0.0)))

    d = _uniform_derivs(rng, n)
    for i in range(n):
        d[i, rng.choice(4, size=int(rng.integers(1, 3)), replace=False)] = 0.0
    put("axis_zero", _st(rng, n), d)

    j = rng.integers(-1, levels + 3, n)
    m = np.where(rng.random(n) < 0.5, np.exp2(-j.astype(np.float64)), np.exp2(-j - 0.5)).astype(f32)
    m = _ulps(m, rng.integers(-2, 3, n))
    d = np.zeros((n, 4), f32)
    shape = rng.integers(0, 4, n)
    half = (m * f32(0.5)).astype(f32)
    d[:, 0] = np.where(shape == 2, half, m); d[:, 3] = np.where(shape == 1, half, m)                   # ds_dx, dt_dy: a square or 2:1 footprint
    swap = shape == 3                                                                                  # the same carried by ds_dy, dt_dx
    d[swap] = d[swap][:, [1, 0, 3, 2]]
    put("lod_boundary", _st(rng, n), d * rng.choice(np.array([-1.0, 1.0], f32), (n, 4)))

    ratio = (np.arange(n) % 17 + 1).astype(f32)
    short = np.exp2(-rng.integers(1, levels + 2, n).astype(np.float64)).astype(f32)
    long_ = _ulps((ratio * short).astype(f32), rng.integers(-1, 2, n))
    put("tap_counts", _st(rng, n), _axes(rng, n, long_, short))

    long_ = np.exp2(-rng.uniform(0, levels, n)).astype(f32)
    short = (long_ / np.exp(rng.uniform(np.log(1e3), np.log(1e6), n))).astype(f32)
    d = _axes(rng, n, long_, short)
    q = max(1, n // 4)                                                          # a quarter: |major axis| == width, exactly and 1 ulp either side
    d[:q] = 0.0
    edge = np.where(rng.random(q) < 0.5, f32(w), f32(h))                       # ... or the height, or between the two: only the width counts
    edge = np.where(rng.random(q) < 0.25, rng.uniform(min(w, h), max(w, h), q), edge).astype(f32)
    d[:q, 0] = _ulps(edge, rng.integers(-1, 2, q)); d[:q, 3] = np.exp(rng.uniform(np.log(1e-4), 0.0, q))
    d[:q:2] = d[:q:2][:, [1, 0, 3, 2]]                                          # ... as the y axis of the footprint too
    put("eccentric", _st(rng, n), d)

    tiny = _ulps(np.full(n, 1e-5, f32), rng.integers(-3, 4, n))
    d = np.zeros((n, 4), f32)
    major = np.exp(rng.uniform(np.log(1e-5), np.log(1e-2), n)).astype(f32)
    diag = rng.random(n) < 0.3
    d[:, 0] = major; d[:, 1] = np.where(diag, tiny * f32(0.70710678), tiny); d[:, 3] = np.where(diag, tiny * f32(0.70710678), 0.0)
    sw = rng.random(n) < 0.5
    d[sw] = d[sw][:, [1, 0, 3, 2]]
    put("minor_tiny", _st(rng, n), d)

    sd = np.array([np.inf, -np.inf, np.nan, 1e38, -1e38, 1e-30, -0.0], f32)
    d = _uniform_derivs(rng, n)
    for i in range(n):
        c = rng.choice(4, size=int(rng.integers(1, 5)), replace=False)
        d[i, c] = sd[rng.integers(len(sd), size=len(c))]
    put("special_deriv", _st(rng, n), d)

    in6 = np.concatenate([parts[c] for c in CLASSES]).astype(f32)
    labels = np.concatenate([np.full(len(parts[c]), c) for c in CLASSES])
    return in6, labels


def fetch_counts(tex, in6, threads=8):
    """(len(CONFIGS), N) oracle texel fetches of each sample under each sampler configuration."""
    import orc
    return np.stack([orc.texture_sample(tex, in6, *cfg, threads=threads)[1] for cfg in CONFIGS.values()])


def generate(tex, n=64, seed=0, threads=8):
    """samples() minus the rows that cost more than MAX_FETCHES oracle texel fetches in any configuration."""
    in6, labels = samples(tex, n, seed)
    keep = (fetch_counts(tex, in6, threads) <= MAX_FETCHES).all(axis=0)
    for c in CLASSES:
        dropped = int((~keep & (labels == c)).sum())
        assert dropped * 100 < int((labels == c).sum()), f"class {c}: {dropped} of {int((labels == c).sum())} samples exceed {MAX_FETCHES} fetches"
    return in6[keep], labels[keep]


def label_index(labels):
    return np.array([CLASSES.index(x) for x in labels], np.int8)


# ---- sky -------------------------------------------------------------------------------------------------------------------------------
SKY_CLASSES = ("axes", "near_poles", "beyond_unit", "degenerate", "index_edges", "unit")


def sky_directions(seed=0, n=64):
    """(dirs (N, 3) float32, labels): the six axes; directions 1 ulp (and a few) off the poles; unnormalised ones with |z| > 1 (acos: NaN);
    the zero vector, inf and NaN components; directions whose (u, v) land on 0, on `size` and on the clamp (z = -1 with a non-zero x or y:
    acos = pi, so u or v reaches 0 or 1 exactly and the index reaches size * size and beyond); random unit directions."""
    rng = np.random.default_rng(seed)
    parts = {}
    parts["axes"] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.0, -0.0, 1], [-0.0, 0.0, -1]], f32)
    near = []
    for z in (1.0, -1.0):
        for k in range(1, 5):
            zz = _ulps(f32(z), -k)
            r = np.sqrt(max(0.0, 1.0 - float(zz) ** 2)); a = rng.uniform(0, 2 * np.pi)
            near += [[r * np.cos(a), r * np.sin(a), zz], [1e-30, 0, z], [0, -1e-38, z], [1e-45, 1e-45, z], [r, 0, zz], [0, -r, zz]]
    parts["near_poles"] = np.array(near, f32)
    b = rng.normal(size=(n, 3)); b[:, 2] = rng.choice([-1, 1], n) * rng.uniform(1.0000001, 3.0, n)
    parts["beyond_unit"] = b.astype(f32)
    sp = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 1e38, 1e-45], f32)
    d = rng.normal(size=(n, 3)).astype(f32)
    for i in range(n):
        c = rng.choice(3, size=int(rng.integers(1, 4)), replace=False)
        d[i, c] = sp[rng.integers(len(sp), size=len(c))]
    d[0] = 0.0
    parts["degenerate"] = d
    e = []
    for x, y in [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1), (3, 0), (0, 2.5), (1e-3, 1), (1, 1e-3)]:
        for z in (-1.0, _ulps(f32(-1.0), -1), _ulps(f32(-1.0), 1)):
            e.append([x, y, z])
    parts["index_edges"] = np.array(e, f32)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    parts["unit"] = u.astype(f32)
    dirs = np.concatenate([parts[c] for c in SKY_CLASSES]).astype(f32)
    return dirs, np.concatenate([np.full(len(parts[c]), c) for c in SKY_CLASSES])


def sky_probe(size, seed=3):
    return np.random.default_rng([seed, size]).uniform(0.05, 1.0, (size, size, 3)).astype(f32)
