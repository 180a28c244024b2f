"""Seeded edit sequences for a long-lived context: sequence(seed) -> the steps, each an edit of a SHADOW scene and one observation.

The shadow scene is a scene_io.Scene (a 64 x 48 cut of the `materials_aniso` golden, its instances posed anew so that they can be moved) plus
what the edits need beside it — the poses, per new BLAS id the source mesh and its slot table, the object masks — and it is advanced on the
host only by the twins of the device calls: host.scene_update_balanced (rtx_update_instances), host.blas_build_balanced (rtx_alloc_blas +
rtx_build_blas, and the meshes that are uploaded), host.blas_refit, host.vertex_normals (the normals a refit hands in),
host.texture_with_mips (rtx_alloc_texture + rtx_update_texture).  Every step keeps a snapshot of the shadow scene after its edit: arrays are
replaced, never written in place, so a snapshot is a shallow copy.

Nothing here needs a GPU.  tests/test_grow_sequences_cpu.py pins the generator (deterministic, legal scenes, coverage of the growth kinds);
tests/test_gpu_grow.py applies the steps to one context and compares every observation with a fresh context, the host twins or the oracle.
All data is finite and legal: no step is meant to be refused.
"""
import copy
import hashlib
import os

import numpy as np

import hitset
import pointset
import sweepset
import util
from test_blas_build_cpu import mesh_as_indexed, soup
from test_blas_refit_cpu import deform

f32 = np.float32
WIDTH, HEIGHT = 64, 48
ROWS = 128                                                   # at most this many rows per query observation

# the edits.  TABLE: the device table of the context that the edit makes larger (include/rtx.h: "scene data that lives across frames")
KINDS = ("blas_upload", "blas_build", "blas_reupload", "blas_refit", "update_instances", "texture", "materials_same", "materials_more", "sky",
         "masks", "set_frame")
TABLE = {"blas_upload": "blas", "blas_build": "blas", "texture": "textures", "materials_more": "materials", "sky": "sky"}
WEIGHTS = (3, 4, 2, 4, 2, 4, 2, 3, 3, 3, 3)
RENDERS = ("render", "render_views", "render_rays", "render_aovs")
QUERIES = ("closest", "occluded", "nearest", "hits", "sweep", "signed")
FILTERED = ("nearest", "hits", "sweep", "signed")          # the queries that take mask=
MESHES = ("soup5", "soup33", "soup257", "Cube", "Diamond", "Torus")
TEXTURE_SHAPES = ((64, 16), (32, 32), (8, 8), (16, 64), (1, 1))        # (w, h): powers of two, a chain each
SKY_SIZES = (16, 32, 48, 64, 128)


def default_seeds():
    """6 seeds; RTX_SEQ_SEEDS=n: the first n (a soak, like RTX_FUZZ_SEEDS)"""
    return list(range(int(os.environ.get("RTX_SEQ_SEEDS", "6"))))


def small(sc, width=WIDTH, height=HEIGHT):
    """The scene's own view pyramid over width x height pixels."""
    sc = copy.copy(sc)
    kx, ky = f32(sc.width / width), f32(sc.height / height)
    sc.config = sc.config.copy(); sc.config["width"] = width; sc.config["height"] = height
    sc.camera = sc.camera.copy()
    sc.camera["rotated_x_axis"] *= kx; sc.camera["rotated_y_axis"] *= ky
    return sc


def materials_scene():
    """materials_aniso at 64 x 48: textures, dielectrics, a plane, two spheres; rays reach the sky"""
    return small(util.load_golden("materials_aniso")[0])


_source = {}


def source_mesh(name):
    """-> (positions (V, 3), indices (T, 3), normals, texcoords, material ids in 0 .. 2), once per run"""
    if name not in _source:
        if name.startswith("soup"):
            pos, idx, nrm, uv, mid = soup(int(name[4:]), 7)
            pos = (pos * f32(0.25)).astype(f32)                                 # the soups span 8 units: a quarter is the size of the scene's meshes
        else:
            pos, idx, nrm, uv, mid = mesh_as_indexed(name)
            mid = (np.arange(len(idx)) % 3).astype(np.int32)
        _source[name] = tuple(np.ascontiguousarray(a) for a in (pos, idx, nrm, uv, mid))
    return _source[name]


class Step:
    """One edit and one observation.  kind + args: the edit (arrays the device call is given); scene, masks: the shadow after it; mesh: the
    (blas, slot vertices, order, positions, indices) of a BLAS the edit made from a source mesh, else None; observe: {"kind", "sort", "mask",
    "rows"}; grows: the table the edit made larger, or None."""

    def __init__(self, kind, args, scene, masks, observe, mesh=None):
        self.kind, self.args, self.scene, self.masks, self.observe, self.mesh = kind, args, scene, masks, observe, mesh
        self.grows = TABLE.get(kind)


class Shadow:
    def __init__(self, seed):
        from pyrtx import host
        self.rng = np.random.default_rng([0x9a0, seed])
        sc = materials_scene()
        n = len(sc.instances)
        self.pos = np.stack([pointset._xform(sc.instances["world"][i], np.zeros((1, 3)))[0] for i in range(n)]).astype(f32)
        self.rot = np.tile(f32([0, 0, 0, 1]), (n, 1))
        sc.blas = list(sc.blas); sc.textures = list(sc.textures)
        sc.instances, sc.tlas_nodes, sc.tlas_indices = host.scene_update_balanced(sc, self.pos, self.rot)
        self.scene = sc
        self.meshes = {}                                     # new BLAS id -> {"name", "pos", "sv", "order", "bound"}: what a refit needs
        self.masks = None
        self.instanced = set()                               # new ids that have an instance

    # ---- helpers ----------------------------------------------------------------------------------------------------------------------
    def snapshot(self):
        s = copy.copy(self.scene)
        s.blas = list(self.scene.blas); s.textures = list(self.scene.textures)
        return s

    def object_count(self):
        return len(self.scene.instances) + len(self.scene.spheres) + len(self.scene.planes)

    def quaternion(self, spread=1.0):
        q = np.array([0, 0, 0, 1.0]) + spread * self.rng.normal(size=4)
        return (q / np.linalg.norm(q)).astype(f32)

    def centre(self):
        """a point in front of the camera, among the scene's objects"""
        return (self.pos[:5].mean(axis=0) + self.rng.uniform(-1.5, 1.5, 3)).astype(f32)

    def twin(self, name, positions, material_offset):
        from pyrtx import host
        _, idx, nrm, uv, mid = source_mesh(name)
        return host.blas_build_balanced(positions, idx, nrm, uv, mid, material_offset)

    def moved(self, name, positions):
        kind = ("twist", "wave", "noise")[int(self.rng.integers(3))]
        return np.ascontiguousarray(deform(positions, kind, int(self.rng.integers(1 << 30)), 0.5), f32)

    # ---- the edits: each returns (args, mesh or None) and leaves self.scene replaced, never written in place ----------------------------
    def blas_new(self, built):
        name = MESHES[int(self.rng.integers(len(MESHES)))]
        pos = source_mesh(name)[0]
        offset = int(self.rng.integers(0, len(self.scene.materials) - 2))       # local ids 0 .. 2
        blas, sv, order = self.twin(name, pos, offset)
        bid = len(self.scene.blas)
        self.scene.blas = self.scene.blas + [blas]
        self.meshes[bid] = {"name": name, "pos": pos, "sv": sv, "order": order, "bound": built}
        args = {"id": bid, "blas": blas, "name": name, "positions": pos, "material_offset": offset}
        return args, (blas, sv, order, pos, source_mesh(name)[1])

    def blas_reupload(self):
        bid = sorted(self.meshes)[int(self.rng.integers(len(self.meshes)))]
        m = self.meshes[bid]
        pos = self.moved(m["name"], source_mesh(m["name"])[0])
        blas, sv, order = self.twin(m["name"], pos, self.scene.blas[bid].material_offset)
        self.scene.blas = self.scene.blas[:bid] + [blas] + self.scene.blas[bid + 1:]
        m.update(pos=pos, sv=sv, order=order, bound=False)                      # an upload drops the binding and what alloc_blas made of the id
        return {"id": bid, "blas": blas}, (blas, sv, order, pos, source_mesh(m["name"])[1])

    def blas_refit(self):
        from pyrtx import host
        bid = sorted(self.meshes)[int(self.rng.integers(len(self.meshes)))]
        m = self.meshes[bid]
        pos = self.moved(m["name"], m["pos"])
        nrm = host.vertex_normals(pos, source_mesh(m["name"])[1])
        blas = host.blas_refit(self.scene.blas[bid], m["sv"], pos, nrm)
        self.scene.blas = self.scene.blas[:bid] + [blas] + self.scene.blas[bid + 1:]
        args = {"id": bid, "bind": None if m["bound"] else m["sv"], "positions": pos, "normals": nrm}
        m.update(pos=pos, bound=True)
        return args, None

    def update_instances(self):
        from pyrtx import host
        n = len(self.pos)
        self.pos = (self.pos + self.rng.uniform(-0.3, 0.3, (n, 3))).astype(f32)
        self.rot = np.stack([self.quaternion(0.3) if self.rng.random() < 0.7 else self.rot[i] for i in range(n)]).astype(f32)
        self.scene.instances, self.scene.tlas_nodes, self.scene.tlas_indices = host.scene_update_balanced(self.scene, self.pos, self.rot)
        return {"positions": self.pos.copy(), "rotations": self.rot.copy()}, None

    def texture(self):
        from pyrtx import host
        w, h = TEXTURE_SHAPES[int(self.rng.integers(len(TEXTURE_SHAPES)))]
        level0 = self.rng.uniform(0.0, 1.0, (h, w, 3)).astype(f32)
        tid = len(self.scene.textures)
        self.scene.textures = self.scene.textures + [host.texture_with_mips(level0)]
        return {"id": tid, "width": w, "height": h, "level0": level0}, None

    def materials(self, more):
        mats = self.scene.materials.copy()
        textured = np.flatnonzero(mats["texture_id"] >= 0)
        if self.rng.random() < 0.6 and len(textured):
            mats["texture_id"][textured[int(self.rng.integers(len(textured)))]] = int(self.rng.integers(len(self.scene.textures)))
        else:
            k = int(self.rng.integers(1, len(mats)))
            mats["diffuse"][k] = self.rng.uniform(0, 1, 3).astype(f32); mats["reflection"][k] = self.rng.uniform(0, 0.9, 3).astype(f32)
        if more:
            extra = np.zeros((1, 3, 40)[int(self.rng.integers(3))], mats.dtype)
            extra["diffuse"] = self.rng.uniform(0, 1, (len(extra), 3)).astype(f32); extra["texture_id"] = -1; extra["index_of_refraction"] = 1.0
            mats = np.concatenate([mats, extra])
        self.scene.materials = mats
        return {"materials": mats}, None

    def sky(self):
        from pyrtx import host
        size = int(self.scene.sky.shape[0])
        size = [s for s in SKY_SIZES if s != size][int(self.rng.integers(len(SKY_SIZES) - 1))]
        sky = np.ascontiguousarray(host.synthetic_sky(size) * f32(self.rng.uniform(0.5, 1.5)), f32)
        self.scene.sky = sky
        return {"sky": sky}, None

    def object_masks(self):
        how = ("host", "device", "none")[int(self.rng.integers(3))]
        if how == "none":
            self.masks = None
            return {"how": how, "masks": None}, None
        masks = self.rng.integers(1, 16, self.object_count()).astype(np.uint32)
        masks[int(self.rng.integers(len(masks)))] = 0xFFFFFFFF
        self.masks = masks
        return {"how": how, "masks": masks}, None

    def set_frame(self):
        """one more instance of the newest id without one, else one more sphere; the object masks (set for other counts) are dropped"""
        from pyrtx import host
        from pyrtx import scene_io as sio
        free = [b for b in sorted(self.meshes) if b not in self.instanced]
        if free:
            bid = free[-1]
            self.instanced.add(bid)
            self.pos = np.concatenate([self.pos, self.centre()[None]]).astype(f32)
            self.rot = np.concatenate([self.rot, self.quaternion()[None]]).astype(f32)
            inst = np.zeros(len(self.pos), sio.INSTANCE)
            inst["blas_id"] = np.concatenate([self.scene.instances["blas_id"], [bid]])
            self.scene.instances = inst
            self.scene.instances, self.scene.tlas_nodes, self.scene.tlas_indices = host.scene_update_balanced(self.scene, self.pos, self.rot)
        else:
            ball = np.zeros(1, sio.SPHERE)
            radius = f32(self.rng.uniform(0.2, 0.6))
            ball["center"] = self.centre(); ball["radius_inv"] = f32(1.0) / radius; ball["radius_squared"] = radius * radius
            ball["material_id"] = int(self.rng.integers(1, len(self.scene.materials)))
            self.scene.spheres = np.concatenate([self.scene.spheres, ball])
        dropped = self.masks is not None
        self.masks = None
        return {"drop_masks": dropped, **({"positions": self.pos.copy(), "rotations": self.rot.copy()} if free else {})}, None

    def edit(self, kind):
        if kind in ("blas_reupload", "blas_refit") and not self.meshes:
            kind = "blas_upload"                             # nothing to re-upload or refit yet
        args, mesh = {"blas_upload": lambda: self.blas_new(False), "blas_build": lambda: self.blas_new(True), "blas_reupload": self.blas_reupload,
                      "blas_refit": self.blas_refit, "update_instances": self.update_instances, "texture": self.texture,
                      "materials_same": lambda: self.materials(False), "materials_more": lambda: self.materials(True), "sky": self.sky,
                      "masks": self.object_masks, "set_frame": self.set_frame}[kind]()
        return kind, args, mesh

    # ---- the observation ----------------------------------------------------------------------------------------------------------------
    def observe(self, step_seed):
        rng = self.rng
        kind = (RENDERS + QUERIES)[int(rng.integers(len(RENDERS) + len(QUERIES)))] if rng.random() < 0.8 else RENDERS[0]
        ob = {"kind": kind, "sort": False, "mask": None, "rows": None}
        if kind in RENDERS:
            return ob
        ob["sort"] = bool(rng.integers(2))
        sc = self.scene
        if kind in ("closest", "occluded"):
            from pyrtx import api
            px = rng.choice(sc.width * sc.height, ROWS, replace=False)
            rows = np.ascontiguousarray(api.pinhole_rays(sc.camera[0], sc.width, sc.height).reshape(-1, 18)[px, :6], f32)
            if kind == "occluded":
                rows = np.concatenate([rows, rng.choice(f32([0.5, 2.0, 6.0, 30.0, np.inf]), (ROWS, 1))], axis=1).astype(f32)
        elif kind in ("nearest", "signed"):
            rows = pointset.generate(sc, 100, step_seed)[0]
        elif kind == "hits":
            rows = hitset.generate(sc, 8, step_seed)[0]
        else:
            rows = sweepset.generate(sc, 100, step_seed)[0]
        rows = rows[~np.isnan(rows).any(axis=1)][:ROWS]       # finite, legal rows only (+inf is a legal maximum distance)
        ob["rows"] = np.ascontiguousarray(rows, f32)
        if kind in FILTERED:
            how = int(rng.integers(3))
            if how == 1:
                ob["mask"] = int(rng.integers(1, 16))
            elif how == 2:
                ob["mask"] = rng.integers(0, 16, len(rows)).astype(np.int32)
        return ob


def first_scene():
    """The shadow scene every sequence starts from (no draw goes into it): what the long-lived context is created with."""
    return Shadow(0).snapshot()


def sequence(seed, steps=10):
    """-> [Step, ...]: deterministic per seed"""
    sh = Shadow(seed)
    rng = sh.rng
    p = np.array(WEIGHTS, np.float64) / sum(WEIGHTS)
    out = []
    for k in range(steps):
        kind, args, mesh = sh.edit(KINDS[int(rng.choice(len(KINDS), p=p))])
        out.append(Step(kind, args, sh.snapshot(), None if sh.masks is None else sh.masks.copy(), sh.observe(1000 * seed + k), mesh))
    return out


def _bytes_of(v):
    if isinstance(v, np.ndarray):
        return v.tobytes()
    if isinstance(v, dict):
        return b"".join(k.encode() + _bytes_of(x) for k, x in sorted(v.items()))
    if isinstance(v, (list, tuple)):
        return b"".join(_bytes_of(x) for x in v)
    if hasattr(v, "nodes"):
        return v.nodes.tobytes() + v.tri_hot.tobytes() + v.tri_cold.tobytes() + repr(v.material_offset).encode()
    if hasattr(v, "texels"):
        return v.desc.tobytes() + v.texels.tobytes()
    return repr(v).encode()


def digest(steps):
    """Every byte a sequence hands to a device call or compares an answer with, hashed: equal digests, equal sequences."""
    h = hashlib.sha256()
    for s in steps:
        sc = s.scene
        h.update(_bytes_of([s.kind, s.args, s.masks, s.observe, sc.blas, sc.textures, sc.materials, sc.sky, sc.instances, sc.tlas_nodes,
                            sc.tlas_indices, sc.spheres, sc.planes]))
    return h.hexdigest()


def coverage(sequences):
    """What a set of sequences exercises -> {"kinds": {edit kind: count}, "observed": {observation kind: count}, "after": {table: (render
    observations, query observations) made after a growth of the table with no set_frame since}, "most_growths": the most growths of one
    table within one sequence, "mask_ways": the ways set_object_masks was called}."""
    kinds = {k: 0 for k in KINDS}
    observed = {k: 0 for k in RENDERS + QUERIES}
    after = {t: [0, 0] for t in ("blas", "materials", "textures", "sky")}
    most = 0
    for s in sequences:
        grown = set()
        for st in s:
            kinds[st.kind] += 1
            observed[st.observe["kind"]] += 1
            if st.kind == "set_frame":
                grown.clear()
            if st.grows:
                grown.add(st.grows)
            for t in grown:
                after[t][st.observe["kind"] in QUERIES] += 1
        most = max([most] + [sum(st.grows == t for st in s) for t in after])
    return {"kinds": kinds, "observed": observed, "after": {t: tuple(v) for t, v in after.items()}, "most_growths": most,
            "mask_ways": {st.args["how"] for s in sequences for st in s if st.kind == "masks"}}
