"""Swept-box queries without a GPU (include/rtx.h: rtx_query_sweep_box; the host twin rtxh_query_sweep_box, csrc/rtx_boxsweep_math.h):
  * the ABI, the exports, the Python-side checks, and csrc/boxsweep_check.cpp under the host sanitizers;
  * the candidate functions against a numpy float32 restatement of the header, bit for bit;
  * the walk against the exhaustive search: never earlier, the same answer at an equal t (the same triangle where a BLAS with spatial
    splits holds it in several slots);
  * both against an fp64 anchor under host.sweep_box_bound: the returned primitive's exact gaps at t, and every primitive's gaps at 64
    sample times before t;
  * analytic cases on the golden cube, a sphere from outside and from inside and a plane, also under a rotated pose;
  * a point box against query_closest, t == 0 against query_overlap, cubes between the two balls of query_sweep; masks, two trees, dead rows."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import boxset
import boxsweepset as bs
import hitset
import util
from test_query_sweep_cpu import stack_need
from test_views_cpu import _offline_renderer

REPO = util.REPO
f32 = np.float32
U = 2.0 ** -24
ALL = ("distance", "normal", "object_id", "triangle_id", "axis")
SCENES = ["cube", "coincident", "materials_aniso", "monkey_small"]
_CACHE = {}


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    return a


@pytest.fixture(scope="module")
def host():
    from pyrtx import host as h
    return h


def load_scene(name):
    if name not in _CACHE:
        _CACHE[name] = util.load_golden(name)[0]
    return _CACHE[name]


def row_set(host, name):
    """(scene, rows, labels, walk, exhaustive), once per run: a few hundred rows per scene."""
    key = ("set", name)
    if key not in _CACHE:
        sc = load_scene(name)
        rows, lab = bs.generate(sc, 16, seed=5)
        _CACHE[key] = (sc, rows, lab, host.query_sweep_box(sc, rows, ALL), host.query_sweep_box_exhaustive(sc, rows, ALL))
    return _CACHE[key]


# ---- 1. declarations, the Python layer, the check program ---------------------------------------------------------------------------------
def test_functions_are_declared_exported_and_bound(api, host):
    plain = re.sub(r"/\*.*?\*/", "", open(f"{REPO}/include/rtx.h").read(), flags=re.S)
    assert re.search(r"\bint\s+rtx_query_sweep_box\s*\(", plain) and re.search(r"\bint\s+rtx_query_sweep_box_filtered\s*\(", plain)
    lib = api.load_library()
    exported = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("rtx_query_sweep_box", "rtx_query_sweep_box_filtered"):
        assert re.search(r"\sT\s+" + name + r"\b", exported), name
        assert name in api.EXPORTS and name in api.SWEEP_BOX_EXPORTS and getattr(lib, name).restype is C.c_int
    assert lib.rtx_query_sweep_box.argtypes[2] is C.c_int64 and len(lib.rtx_query_sweep_box.argtypes) == 9 and len(lib.rtx_query_sweep_box_filtered.argtypes) == 10
    host_header = re.sub(r"/\*.*?\*/", "", open(f"{REPO}/include/rtx_host.h").read(), flags=re.S)
    hlib = host.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", hlib._name], capture_output=True, text=True, check=True).stdout
    for name in ("rtxh_query_sweep_box", "rtxh_query_sweep_box_exhaustive", "rtxh_sweep_box_triangle", "rtxh_sweep_box_sphere", "rtxh_sweep_box_plane"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", host_header), name
        assert re.search(r"\sT\s+" + name + r"\b", exported), name
        assert name in host.EXPORTS and getattr(hlib, name).restype is C.c_int
    assert re.search(r"\bfloat\s+rtxh_sweep_box_bound\s*\(", host_header)
    # margin(S, W, kappa) = (192 S kappa + 8 W) u, plus (32 S + (64 + 128 kappa) T) u
    assert host.sweep_box_bound(1.0, 0.0, 0.0, 1.0) == (192 + 32) * U and host.sweep_box_bound(0.0, 1.0, 0.0, 5.0) == 8 * U
    assert host.sweep_box_bound(0.0, 0.0, 1.0, 1.0) == 192 * U and host.sweep_box_bound(0.0, 0.0, 2.0, 3.0) == 896 * U
    assert host.sweep_box_bound(1.0, 0.0, 0.0, 1.0) == host.overlap_margin(1.0, 0.0, 1.0) + 32 * U
    for mk in ("csrc", "host"):
        assert "rtx_boxsweep_math.h" in open(f"{REPO}/cpu-raytracer_amd/{mk}/Makefile").read()
    for header, word in (("rtx_overlap_math.h", "rtx_boxsweep_math.h"),):          # the siblings point here instead of calling swept boxes out of scope
        assert word in open(f"{REPO}/cpu-raytracer_amd/csrc/{header}").read()


def test_python_checks_come_before_the_library(api):
    torch = pytest.importorskip("torch")
    r = _offline_renderer(api)                                          # ctx and lib are None: a call that got through would raise AttributeError
    rows = torch.zeros((8, 14), dtype=torch.float32)
    for kw in ({}, {"channels": ALL, "sort": True}, {"channels": "axis"}, {"channels": ("normal", "distance")}, {"mask": 3}):
        with pytest.raises(ValueError, match="cuda:0"):                 # every check up to the device check passes
            r.query_sweep_box(rows, **kw)
    with pytest.raises(ValueError, match=r"\(n, 14\)"):
        r.query_sweep_box(torch.zeros((8, 10), dtype=torch.float32))
    with pytest.raises(TypeError):
        r.query_sweep_box(rows.double())
    with pytest.raises(TypeError):
        r.query_sweep_box(np.zeros((8, 14), f32))
    with pytest.raises(ValueError, match="unknown channel"):
        r.query_sweep_box(rows, ("distance", "position"))
    with pytest.raises(ValueError, match="at least one"):
        r.query_sweep_box(rows, ())
    with pytest.raises(ValueError, match="twice"):
        r.query_sweep_box(rows, ("axis", "axis"))
    with pytest.raises(ValueError, match="not requested"):
        r.query_sweep_box(rows, "distance", out={"axis": torch.zeros((8,), dtype=torch.int32)})
    with pytest.raises(ValueError, match=r"shape \(8, 3\)"):
        r.query_sweep_box(rows, "normal", out={"normal": torch.zeros((8,))})
    with pytest.raises(ValueError, match=r"shape \(8,\)"):
        r.query_sweep_box(rows, "axis", out={"axis": torch.zeros((8, 1), dtype=torch.int32)})
    with pytest.raises(TypeError):
        r.query_sweep_box(rows, "axis", out={"axis": torch.zeros((8,))})          # float32 where int32 is due
    with pytest.raises(TypeError):
        r.query_sweep_box(rows, "distance", out=[torch.zeros((8,))])
    with pytest.raises(ValueError, match="n is needed"):
        r.query_sweep_box(0x1000)
    with pytest.raises(ValueError, match="every requested channel"):
        r.query_sweep_box(0x1000, ("distance", "axis"), n=8, out={"distance": 0x2000})
    with pytest.raises(ValueError, match="null device pointer"):
        r.query_sweep_box(0x1000, "distance", n=8, out={"distance": 0})
    with pytest.raises(ValueError, match="32 bits"):
        r.query_sweep_box(rows, mask=1 << 40)
    with pytest.raises(ValueError, match=r"n must be in"):
        r.query_sweep_box(rows, n=9)
    with pytest.raises(TypeError):
        r.query_sweep_box(rows, lane_trace=True)


def test_host_twin_refuses_bad_arguments(host):
    sc = load_scene("cube")
    rows = np.stack([c[0] for c in bs.cube_cases()])[:4]
    with pytest.raises(ValueError):
        host.query_sweep_box(sc, rows[:, :10])
    with pytest.raises(TypeError):
        host.query_sweep_box(sc, rows.astype(np.float64))
    with pytest.raises(ValueError):
        host.query_sweep_box(sc, rows, ("distance", "uv"))
    with pytest.raises(ValueError):
        host.query_sweep_box(sc, rows, ())
    lib = host.lib()
    s, keep = host.nearest_scene(sc)
    t = np.zeros(4, f32)
    assert lib.rtxh_query_sweep_box(C.byref(s), rows.ctypes.data, 4, None, None, None, None, None, None, None, None, 0xFFFFFFFF) == 1      # no output
    assert lib.rtxh_query_sweep_box(C.byref(s), None, 4, t.ctypes.data, None, None, None, None, None, None, None, 0xFFFFFFFF) == 1
    assert lib.rtxh_query_sweep_box(C.byref(s), rows.ctypes.data, 0, t.ctypes.data, None, None, None, None, None, None, None, 0xFFFFFFFF) == 1
    assert lib.rtxh_query_sweep_box_exhaustive(C.byref(s), rows.ctypes.data, 4, None, None, None, None, None, None, None, 0xFFFFFFFF) == 1
    assert lib.rtxh_query_sweep_box(C.byref(s), rows.ctypes.data, 4, t.ctypes.data, None, None, None, None, None, None, None, 0xFFFFFFFF) == 0


def test_boxsweep_check_program():
    """csrc/boxsweep_check.cpp: the walk against the exhaustive search on generated trees up to the stack bound, under the host sanitizers."""
    out = subprocess.run(["make", "-B", "-C", os.path.join(REPO, "cpu-raytracer_amd", "csrc"), "boxsweep_check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "boxsweep_check: ok" in out.stdout
    assert re.search(r"deepest stack 6[0-4] of 64", out.stdout)


# ---- 2. the candidate functions against a float32 restatement of the header -----------------------------------------------------------------
def _dot(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def _mn(a, b):
    return a if a < b else b


def _mx(a, b):
    return a if a > b else b


def _frame(row):
    """rtxop::world_frame over (c, h, q) of a 14-float row, in float32 scalars: (c, [a0, a1, a2], h)."""
    r = [f32(v) for v in row]
    c, h, q = r[0:3], r[7:10], r[10:14]
    l = np.sqrt(q[0] * q[0] + (q[1] * q[1] + (q[2] * q[2] + q[3] * q[3])))
    x, y, z, w = q[0] / l, q[1] / l, q[2] / l, q[3] / l
    xx, yy, zz, xz, xy, yz, wx, wy, wz = x * x, y * y, z * z, x * z, x * y, y * z, w * x, w * y, w * z
    one, two = f32(1), f32(2)
    a0 = [one - two * (yy + zz), two * (xy + wz), two * (xz - wy)]
    a1 = [two * (xy - wz), one - two * (xx + zz), two * (yz + wx)]
    a2 = [two * (xz + wy), two * (yz - wx), one - two * (xx + yy)]
    return c, [a0, a1, a2], h


def _to_box(A, d):
    return [_dot(A[0], d), _dot(A[1], d), _dot(A[2], d)]


def _axis_passes(lo, hi, r):
    return bool(lo <= r) and bool(hi >= -r)


def _static_triangle(v0, f1, f2, h):
    v1 = [v0[k] + f1[k] for k in range(3)]; v2 = [v0[k] + f2[k] for k in range(3)]
    ok = all(_axis_passes(_mn(_mn(v0[k], v1[k]), v2[k]), _mx(_mx(v0[k], v1[k]), v2[k]), h[k]) for k in range(3))
    n = [f1[1] * f2[2] - f1[2] * f2[1], f1[2] * f2[0] - f1[0] * f2[2], f1[0] * f2[1] - f1[1] * f2[0]]
    pn = _dot(n, v0)
    ok = ok and _axis_passes(pn, pn, h[0] * abs(n[0]) + (h[1] * abs(n[1]) + h[2] * abs(n[2])))
    if not ok:
        return False

    def edge(f, va, vb):
        ax, ay, az = abs(f[0]), abs(f[1]), abs(f[2])
        def two(pa, pb, r): return _axis_passes(_mn(pa, pb), _mx(pa, pb), r)
        return (two(f[1] * va[2] - f[2] * va[1], f[1] * vb[2] - f[2] * vb[1], h[1] * az + h[2] * ay) and two(f[2] * va[0] - f[0] * va[2], f[2] * vb[0] - f[0] * vb[2], h[0] * az + h[2] * ax)
                and two(f[0] * va[1] - f[1] * va[0], f[0] * vb[1] - f[1] * vb[0], h[0] * ay + h[1] * ax))
    f12 = [f2[k] - f1[k] for k in range(3)]
    return edge(f1, v0, v2) and edge(f12, v1, v0) and edge(f2, v0, v1)


def restated_triangle(row, bound, p0, e1, e2):
    """rtxbs::triangle_sweep at the row's world frame -> None or (t, axis), every operation a float32 one in the header's order."""
    with np.errstate(all="ignore"):
        c, A, h = _frame(row)
        w = _to_box(A, [f32(v) for v in row[3:6]])
        v0 = _to_box(A, [f32(p0[k]) - c[k] for k in range(3)]); f1 = _to_box(A, [f32(v) for v in e1]); f2 = _to_box(A, [f32(v) for v in e2])
        if _static_triangle(v0, f1, f2, h):
            return f32(0), 13
        v1 = [v0[k] + f1[k] for k in range(3)]; v2 = [v0[k] + f2[k] for k in range(3)]
        n1 = lambda a: abs(a[0]) + (abs(a[1]) + abs(a[2]))
        S = {"best": f32(-np.inf), "out": f32(np.inf), "pad": (f32(8) * f32(U)) * ((n1(v0) + (n1(f1) + n1(f2))) + n1(h)), "axis": -1, "ok": True}

        def axis(k, lo, hi, r0, vL, l1):
            r = r0 + S["pad"] * l1
            if vL == 0:
                S["ok"] = S["ok"] and _axis_passes(lo, hi, r); return
            a, b = (lo - r) / vL, (hi + r) / vL
            S["ok"] = S["ok"] and bool(a == a) and bool(b == b)
            en, ex = _mn(a, b), _mx(a, b)
            if en > S["best"]:
                S["best"] = en; S["axis"] = k
            S["out"] = _mn(S["out"], ex)

        def live():
            t_in = _mx(f32(0), S["best"])
            return S["ok"] and bool(t_in <= S["out"] + (f32(32) * f32(U)) * S["out"]) and bool(t_in <= f32(bound))

        def edge(k, f, va, vb):
            ax, ay, az = abs(f[0]), abs(f[1]), abs(f[2])
            a0, b0 = f[1] * va[2] - f[2] * va[1], f[1] * vb[2] - f[2] * vb[1]
            axis(k, _mn(a0, b0), _mx(a0, b0), h[1] * az + h[2] * ay, f[1] * w[2] - f[2] * w[1], ay + az)
            a1, b1 = f[2] * va[0] - f[0] * va[2], f[2] * vb[0] - f[0] * vb[2]
            axis(k + 1, _mn(a1, b1), _mx(a1, b1), h[0] * az + h[2] * ax, f[2] * w[0] - f[0] * w[2], ax + az)
            a2, b2 = f[0] * va[1] - f[1] * va[0], f[0] * vb[1] - f[1] * vb[0]
            axis(k + 2, _mn(a2, b2), _mx(a2, b2), h[0] * ay + h[1] * ax, f[0] * w[1] - f[1] * w[0], ax + ay)
        for k in range(3):
            axis(k, _mn(_mn(v0[k], v1[k]), v2[k]), _mx(_mx(v0[k], v1[k]), v2[k]), h[k], w[k], f32(1))
        n = [f1[1] * f2[2] - f1[2] * f2[1], f1[2] * f2[0] - f1[0] * f2[2], f1[0] * f2[1] - f1[1] * f2[0]]
        pn = _dot(n, v0)
        axis(3, pn, pn, h[0] * abs(n[0]) + (h[1] * abs(n[1]) + h[2] * abs(n[2])), _dot(n, w), n1(n))
        if not live(): return None
        edge(4, f1, v0, v2)
        if not live(): return None
        edge(7, [f2[k] - f1[k] for k in range(3)], v1, v0)
        if not live(): return None
        edge(10, f2, v0, v1)
        if not live() or S["axis"] < 0: return None
        return _mx(f32(0), S["best"]), S["axis"]


def restated_plane(row, n, distance):
    with np.errstate(all="ignore"):
        c, A, h = _frame(row)
        n = [f32(v) for v in n]; d = [f32(v) for v in row[3:6]]
        s = _dot(n, c) + f32(distance)
        r = h[0] * abs(_dot(n, A[0])) + (h[1] * abs(_dot(n, A[1])) + h[2] * abs(_dot(n, A[2])))
        if abs(s) <= r:
            return f32(0)
        g = _dot(n, d)
        a = -g if s > 0 else g
        if not a > 0:
            return None
        return (abs(s) - r) / a


def _approach(m, d, q2):
    dd = _dot(d, d)
    tc = -_dot(m, d) / dd
    k = [m[i] + d[i] * tc for i in range(3)]
    w = (q2 - _dot(k, k)) / dd
    if not w >= 0:
        return None
    return tc, np.sqrt(w)


def restated_sphere(row, bound, center, R2):
    """rtxbs::sphere_sweep at the row's world frame -> None or t."""
    with np.errstate(all="ignore"):
        c, A, h = _frame(row)
        w = _to_box(A, [f32(v) for v in row[3:6]])
        x = _to_box(A, [f32(center[k]) - c[k] for k in range(3)])
        R2, bound, zero, inf = f32(R2), f32(bound), f32(0), f32(np.inf)
        near = [_mx(abs(x[k]) - h[k], zero) for k in range(3)]; far = [abs(x[k]) + h[k] for k in range(3)]
        dmin2, dmax2 = near[0] * near[0] + (near[1] * near[1] + near[2] * near[2]), far[0] * far[0] + (far[1] * far[1] + far[2] * far[2])
        if dmin2 <= R2 and R2 <= dmax2:
            return zero
        if not _dot(w, w) > 0:
            return None
        sign = lambda v, fb: f32(1) if v > 0 else f32(-1) if v < 0 else f32(-1) if fb < 0 else f32(1)
        sg = [sign(w[k], x[k]) for k in range(3)]
        if dmin2 > R2:
            tin, tout = [], []
            for k in range(3):
                if w[k] == 0:
                    tin.append(-inf if abs(x[k]) <= h[k] else inf); tout.append(inf)
                else:
                    a, b = (x[k] - h[k]) / w[k], (x[k] + h[k]) / w[k]
                    tin.append(_mn(a, b)); tout.append(_mx(a, b))
            T = sorted([tin[0], tout[0], tin[1], tout[1], tin[2], tout[2]])
            for j in range(7):
                S, E = (-inf if j == 0 else T[j - 1]), (inf if j == 6 else T[j])
                if E < 0: continue
                S0 = _mx(S, zero)
                if S0 > bound: return None
                m, v = [], []
                for k in range(3):
                    behind = bool(S >= tout[k]); within = (not behind) and bool(S >= tin[k])
                    m.append(zero if within else x[k] + sg[k] * h[k] if behind else x[k] - sg[k] * h[k])
                    v.append(zero if within else -w[k])
                ap = _approach(m, v, R2)
                if ap is None: continue
                tc, sq = ap
                tr = tc - sq
                if tr < S0:
                    if tc + sq >= S0: return S0
                    continue
                if tr <= E: return tr
            return None
        z = [inf if w[k] == 0 else x[k] / w[k] for k in range(3)]
        Z = sorted(z)
        for j in range(4):
            S, E = (-inf if j == 0 else Z[j - 1]), (inf if j == 3 else Z[j])
            if E < 0: continue
            S0 = _mx(S, zero)
            if S0 > bound: return None
            m = [x[k] - sg[k] * h[k] if S >= z[k] else x[k] + sg[k] * h[k] for k in range(3)]
            ap = _approach(m, [-w[0], -w[1], -w[2]], R2)
            if ap is None: return S0
            tr = ap[0] + ap[1]
            if tr < S0: return S0
            if tr <= E: return tr
        return None


def same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


def test_candidate_functions_against_the_restated_header(host):
    from pyrtx import scene_io as sio
    lib = host.lib()
    rng = np.random.default_rng(17)
    sc, rows, lab, w, e = row_set(host, "materials_aniso")
    live = rows[~bs.is_dead(rows)]
    hot_all = [(inst, sc.blas[int(inst["blas_id"])].tri_hot) for inst in sc.instances if np.array_equal(np.asarray(inst["world"], f32).reshape(4, 4), np.eye(4, dtype=f32))]
    cube = load_scene("cube").blas[0].tri_hot
    checked = {"tri": 0, "tri_hit": 0, "axes": set(), "sphere": 0, "sphere_hit": 0, "plane": 0, "plane_hit": 0}
    cases = [(c[0], cube) for c in bs.cube_cases()] + [(r, cube) for r in row_set(host, "cube")[1][~bs.is_dead(row_set(host, "cube")[1])][::2]]
    for r in live[::3]:
        if hot_all:
            cases.append((r, hot_all[int(rng.integers(len(hot_all)))][1]))
    for r, hot in cases:
        r = np.ascontiguousarray(r, f32)
        for j in rng.permutation(len(hot))[:6]:
            tri = np.zeros(1, sio.TRI_HOT); tri[0] = hot[j]
            for bound in (np.inf, 0.5):
                t, ax = C.c_float(0), C.c_int32(-1)
                got = lib.rtxh_sweep_box_triangle(r.ctypes.data, C.c_float(bound), tri.ctypes.data, C.byref(t), C.byref(ax))
                want = restated_triangle(r, bound, hot["position_0"][j], hot["position_edge_1"][j], hot["position_edge_2"][j])
                assert bool(got) == (want is not None), (r, j, bound, got, want)
                checked["tri"] += 1
                if want is not None:
                    assert same_bits(t.value, want[0]) and ax.value == want[1], (r, j, t.value, ax.value, want)
                    checked["tri_hit"] += 1; checked["axes"].add(want[1])
    SPH, PLN = sio.SPHERE if hasattr(sio, "SPHERE") else None, sio.PLANE if hasattr(sio, "PLANE") else None
    spheres = list(sc.spheres) + list(hitset.quad_stack_scene().spheres)
    planes = list(sc.planes) + list(hitset.quad_stack_scene().planes)
    more = bs.generate(hitset.quad_stack_scene(), 8, seed=9)[0]
    for r in np.concatenate([live, more[~bs.is_dead(more)]]):
        r = np.ascontiguousarray(r, f32)
        for s in spheres:
            one = np.zeros(1, sc.spheres.dtype); one[0] = s
            for bound in (np.inf, 1.0):
                t = C.c_float(0)
                got = lib.rtxh_sweep_box_sphere(r.ctypes.data, C.c_float(bound), one.ctypes.data, C.byref(t))
                want = restated_sphere(r, bound, s["center"], s["radius_squared"])
                assert bool(got) == (want is not None), (r, bound, got, want)
                checked["sphere"] += 1
                if want is not None:
                    assert same_bits(t.value, want), (r, t.value, want); checked["sphere_hit"] += 1
        for p in planes:
            one = np.zeros(1, sc.planes.dtype); one[0] = p
            t = C.c_float(0)
            got = lib.rtxh_sweep_box_plane(r.ctypes.data, one.ctypes.data, C.byref(t))
            want = restated_plane(r, p["normal"], p["distance"])
            assert bool(got) == (want is not None), (r, got, want)
            checked["plane"] += 1
            if want is not None:
                assert same_bits(t.value, want), (r, t.value, want); checked["plane_hit"] += 1
    print(checked)
    assert checked["tri_hit"] > 100 and checked["sphere_hit"] > 100 and checked["plane_hit"] > 100 and {0, 3, 13} <= checked["axes"] and len(checked["axes"] & set(range(4, 13))) >= 3


# ---- 3. the walk against the exhaustive search ----------------------------------------------------------------------------------------------
def has_splits(sc, obj):
    """Whether object obj's BLAS stores some triangle in more than one slot (the spatial splits of the reference's SBVH)."""
    key = ("splits", id(sc), int(sc.instances[obj]["blas_id"]))
    if key not in _CACHE:
        hot = sc.blas[int(sc.instances[obj]["blas_id"])].tri_hot
        flat = np.concatenate([hot["position_0"], hot["position_edge_1"], hot["position_edge_2"]], axis=1)
        _CACHE[key] = len(np.unique(flat, axis=0)) < len(flat)
    return _CACHE[key]


def same_triangle(sc, obj, a, b):
    """Whether slots a and b of object obj hold one triangle (a BLAS with spatial splits stores a triangle once per leaf it reaches)."""
    hot = sc.blas[int(sc.instances[obj]["blas_id"])].tri_hot
    return all(np.array_equal(hot[k][a], hot[k][b]) for k in ("position_0", "position_edge_1", "position_edge_2"))


# rows whose equal t names ANOTHER triangle than the exhaustive search's (split leaves, an exact tie at a shared vertex): the counts seen
OTHER_TRIANGLE = {"cube": 0, "coincident": 0, "materials_aniso": 0, "monkey_small": 2}


@pytest.mark.parametrize("name", SCENES)
def test_walk_against_exhaustive_search(host, name):
    sc, rows, lab, w, e = row_set(host, name)
    n = len(rows)
    assert 200 <= n <= 400
    dead = bs.is_dead(rows)
    assert (dead == (lab == bs.CLASSES.index("dead"))).all()
    for out in (w, e):
        assert np.isinf(out["distance"][dead]).all() and (out["object_id"][dead] == -1).all() and (out["triangle_id"][dead] == -1).all() and (out["axis"][dead] == -1).all() and not out["normal"][dead].any()
        assert not np.isfinite(out["distance"][bs.in_classes(lab, ("free", "plane_from"))]).any()
        hit = np.isfinite(out["distance"])
        assert (out["distance"][hit] >= 0).all() and (out["distance"][hit] < rows[hit, 6]).all() and ((out["object_id"] >= 0) == hit).all() and ((out["axis"] >= 0) == hit).all()
        assert ((out["axis"] == 13) <= (out["distance"] == 0)).all()
        assert ((out["triangle_id"] >= 0) == (hit & (out["object_id"] < len(sc.instances)))).all()
    assert not (w["distance"] < e["distance"]).any(), "the walk is earlier than the exhaustive search"
    later = w["distance"] > e["distance"]
    equal = ~later
    moved = other = 0
    for i in np.flatnonzero(equal & np.isfinite(w["distance"])):
        assert w["object_id"][i] == e["object_id"][i] and w["axis"][i] == e["axis"][i], (name, i)
        if w["triangle_id"][i] != e["triangle_id"][i]:
            # a BLAS with spatial splits (monkey_small): another slot of the same triangle, or a triangle that ties exactly (a shared vertex
            # or edge) whose lower slot lies under a leaf box that holds only the part of it the box does not reach (SPLIT LEAVES)
            assert has_splits(sc, int(w["object_id"][i])), (name, i, w["triangle_id"][i], e["triangle_id"][i])
            moved += 1
            if not same_triangle(sc, w["object_id"][i], w["triangle_id"][i], e["triangle_id"][i]):
                # the equal t IS the tie: both searches computed their triangle's candidate by the same function.  The two must share a vertex
                other += 1
                hot = sc.blas[int(sc.instances[int(w["object_id"][i])]["blas_id"])].tri_hot
                verts = lambda j: {tuple(v) for v in (hot["position_0"][j], hot["position_0"][j] + hot["position_edge_1"][j], hot["position_0"][j] + hot["position_edge_2"][j])}
                assert verts(int(w["triangle_id"][i])) & verts(int(e["triangle_id"][i])), (name, i, w["triangle_id"][i], e["triangle_id"][i])
            continue
        assert np.array_equal(w["normal"][i], e["normal"][i])
    print(f"{name}: {n} rows, {int(np.isfinite(w['distance']).sum())} answered, {int((w['distance'] == 0).sum())} at t = 0, {int(later.sum())} later than the exhaustive search, {moved} through another slot, {other} of them another triangle that ties, stack {w['stack_max']}")
    assert later.sum() * 50 <= n
    assert other <= OTHER_TRIANGLE[name], (name, other)
    assert np.isfinite(w["distance"][bs.in_classes(lab, ("approach", "face_on", "d_inf", "zero3"))]).mean() > 0.8      # a tilted flight may slide past the mesh's rim
    assert (w["distance"][bs.in_classes(lab, ("overlap", "touch"))] == 0).all()
    # D just below the contact: unanswered by this primitive (a later t or none); just above: the same answer
    pos = np.flatnonzero(np.isfinite(w["distance"]) & (w["distance"] > 0))[:60]
    below, above = bs.d_rows(rows[pos], w["distance"][pos])
    b = host.query_sweep_box(sc, below, ALL); a = host.query_sweep_box(sc, above, ALL)
    assert not np.isfinite(b["distance"]).any() and all(np.array_equal(a[k], w[k][pos]) for k in ALL)
    at = rows[pos].copy(); at[:, 6] = w["distance"][pos]
    assert not np.isfinite(host.query_sweep_box(sc, at, "distance")["distance"]).any(), "t < D is strict"
    assert w["stack_max"] <= stack_need(sc), (w["stack_max"], stack_need(sc))


def test_axis_classes_on_a_lone_triangle(host):
    """Face on: a box axis.  A corner onto the face: the normal.  Edge against edge: each of the nine cross axes at least once."""
    tri = np.array([[[0.0, 0.0, 0.0], [2.0, 0.25, 0.0], [0.5, 1.75, 0.25]]])
    sc = hitset.mesh_scene([tri])
    rows, lab = bs.generate(sc, 60, seed=2)
    w = host.query_sweep_box(sc, rows, ALL)
    ax = lambda name: w["axis"][bs.in_classes(lab, (name,))]
    # face on: the box axis, the normal and the six cross axes of the two in-plane box axes all point along the normal and tie up to rounding
    assert np.isin(ax("face_on"), (0, 3, 5, 6, 8, 9, 11, 12)).all() and (ax("face_on") == 0).sum() >= 10, np.unique(ax("face_on"), return_counts=True)
    z3 = ax("zero3")
    assert (ax("approach") == 3).sum() >= 10 and (z3[z3 >= 0] == 3).all() and (z3 == 3).sum() >= 30      # a corner, and a point, onto the face: the normal
    seen = set(ax("edge_edge").tolist())
    assert set(range(4, 13)) <= seen, sorted(seen)
    vf = ax("vertex_face")
    assert np.isin(vf, (0, 1, 2)).mean() > 0.5
    par = w["distance"][bs.in_classes(lab, ("parallel",))]
    assert not np.isfinite(par).any(), "hovering over the face and moving along it touches nothing"


# ---- 4. the fp64 anchor ---------------------------------------------------------------------------------------------------------------------
def sliver(hot, t):
    e1, e2 = hot["position_edge_1"][t].astype(np.float64), hot["position_edge_2"][t].astype(np.float64)
    n = np.linalg.norm(np.cross(e1, e2))
    return n == 0 or np.linalg.norm(e1) * np.linalg.norm(e2) / n > 4


def world_triangles(sc):
    """Per instance: (centroids (T, 3), radii (T,)) of its triangles in world space, fp64; once per scene."""
    key = ("worldtris", id(sc))
    if key not in _CACHE:
        out = []
        for inst in sc.instances:
            hot = sc.blas[int(inst["blas_id"])].tri_hot
            p0, e1, e2 = (hot[k].astype(np.float64) for k in ("position_0", "position_edge_1", "position_edge_2"))
            v = np.stack([hitset._xform(inst["world"], p0), hitset._xform(inst["world"], p0 + e1), hitset._xform(inst["world"], p0 + e2)], axis=1)
            with np.errstate(invalid="ignore"):
                cen = v.mean(axis=1)
                out.append((cen, np.linalg.norm(v - cen[:, None, :], axis=2).max(axis=1)))
        _CACHE[key] = out
    return _CACHE[key]


@pytest.mark.parametrize("name", SCENES)
def test_fp64_anchor_under_the_bound(host, name):
    """For the walk AND the exhaustive search, every row answered by a triangle: at the returned t the returned triangle's exact maximal gap
    lies within sweep_box_bound of 0; and at 64 times before t no triangle has every gap below -sweep_box_bound(..., 1) — tested on the
    triangles whose bounding sphere comes within the box's circumscribed radius of the path, the only ones that can reach the box (a
    triangle farther away has a positive gap on some axis).  Rows the bound excludes (the winning axis with kappa beyond 2^10, the normal
    axis of a sliver) are left out of the first check: at most 5 % of the answered rows."""
    sc, rows, lab, w, e = row_set(host, name)
    ni = len(sc.instances)
    wt = world_triangles(sc)
    left_out = checked = sampled = pairs = 0
    classes = set()
    dl = np.linalg.norm(rows[:, 3:6].astype(np.float64), axis=1)
    for out in (w, e):
        for i in np.flatnonzero(np.isfinite(out["distance"]) & (out["object_id"] < ni) & (out["object_id"] >= 0)):
            t, obj, slot = float(out["distance"][i]), int(out["object_id"][i]), int(out["triangle_id"][i])
            S, W, kap, k, cos, excluded, _, gap = bs.contact(sc, rows[i], t, obj, slot, out["normal"][i])
            if excluded:
                left_out += 1
            else:
                bound = host.sweep_box_bound(S, W, t * dl[i], kap)
                assert (abs(gap) <= bound) if t > 0 else (gap <= bound), (name, i, bs.CLASSES[lab[i]], t, gap, bound, k, kap)
                checked += 1
            if t == 0 or (out is e and e["distance"][i] == w["distance"][i]):
                continue                                                        # the same row and the same t: checked with the walk
            # nothing penetrates deeper than the bound before t
            sampled += 1; classes.add(bs.CLASSES[lab[i]])
            c0, d = rows[i, 0:3].astype(np.float64), rows[i, 3:6].astype(np.float64)
            reach = float(np.linalg.norm(rows[i, 7:10].astype(np.float64)))
            for k2, inst2 in enumerate(sc.instances):
                cen, rad = wt[k2]
                with np.errstate(invalid="ignore"):
                    along = np.clip((cen - c0) @ d / (d @ d), 0.0, t)
                    near = np.flatnonzero(np.linalg.norm(cen - (c0 + along[:, None] * d), axis=1) <= (reach + rad) * 1.001 + 1e-6)
                if not len(near):
                    continue
                hot2 = sc.blas[int(inst2["blas_id"])].tri_hot[near]
                for tp in np.linspace(0.0, t, 66)[1:-1]:
                    g2, kap2, S2, W2 = bs.gaps_at(rows[i], tp, inst2, hot2)
                    worst = g2.max(axis=1)
                    for j in np.flatnonzero(worst < 0):                         # only a triangle that penetrates at all needs its bound
                        pairs += 1
                        assert worst[j] >= -host.sweep_box_bound(float(S2[j]), W2, tp * dl[i], 1.0), (name, i, bs.CLASSES[lab[i]], tp, t, int(near[j]), float(worst[j]))
    print(f"{name}: {checked} answers within the bound, {left_out} left out, {sampled} rows sampled at 64 times ({pairs} penetrating pairs met), classes {sorted(classes)}")
    assert checked > 150 and left_out * 20 <= checked + left_out and sampled >= 60 and len(classes) >= 8


# ---- 5. analytic cases ------------------------------------------------------------------------------------------------------------------------
def test_analytic_cube_cases(host):
    sc = load_scene("cube")
    cases = bs.cube_cases()
    rows = np.stack([c[0] for c in cases])
    for ex in (False, True):
        out = (host.query_sweep_box_exhaustive if ex else host.query_sweep_box)(sc, rows, ALL)
        for i, (r, t, axes, nrm) in enumerate(cases):
            T = 0.0 if t is None or not np.isfinite(t) else t * float(np.linalg.norm(r[3:6]))
            tol = host.sweep_box_bound(8.0, 0.0, T, 1.0) / float(np.linalg.norm(r[3:6]))      # head on: the gap closes at |d| per unit of t
            if t is not None:
                assert (np.isinf(out["distance"][i]) if np.isinf(t) else abs(float(out["distance"][i]) - t) <= tol), (ex, i, float(out["distance"][i]), t, tol)
            assert int(out["axis"][i]) in axes, (ex, i, int(out["axis"][i]), axes)
            if nrm is not None:
                assert np.allclose(out["normal"][i], nrm, atol=1e-6), (ex, i, out["normal"][i], nrm)
            assert (out["object_id"][i] == 0) == bool(np.isfinite(out["distance"][i]))


def test_grazing_passes_miss_and_hit_by_multiples_of_the_bound(host):
    """A box flying along the cube's face x = 1: clear of it by 4, 16 and 256 bounds it passes; biting by as much it stops at the face y = -1."""
    sc = load_scene("cube")
    B = host.sweep_box_bound(8.0, 0.0, 6.0, 1.0)
    gaps = [4 * B, 16 * B, 256 * B, -4 * B, -16 * B, -256 * B]
    rows = bs.graze_rows(gaps)
    assert (rows[:3, 0] > 1.25).all() and (rows[3:, 0] < 1.25).all()
    for ex in (False, True):
        out = (host.query_sweep_box_exhaustive if ex else host.query_sweep_box)(sc, rows, ALL)
        assert np.isinf(out["distance"][:3]).all() and (out["axis"][:3] == -1).all(), (ex, out["distance"])
        assert np.allclose(out["distance"][3:], 1.5, atol=1e-4) and (out["axis"][3:] == 1).all() and np.allclose(out["normal"][3:], (0.0, -1.0, 0.0), atol=1e-6), (ex, out["distance"], out["axis"])


def test_analytic_cases_under_a_rotated_pose(host):
    """The cube under CUBE_POSE: rows given in the cube's own frame and posed with it answer as they do for the unmoved cube."""
    sc = hitset.cube_pose_scene()
    pos, rot = hitset.CUBE_POSE
    m = np.asarray(sc.instances[0]["world"], np.float64).reshape(4, 4)
    cases = bs.cube_cases()
    local = np.stack([c[0] for c in cases]).astype(np.float64)
    posed = local.copy()
    posed[:, 0:3] = local[:, 0:3] @ m[:3, :3].T + m[:3, 3]
    posed[:, 3:6] = local[:, 3:6] @ m[:3, :3].T
    for i in range(len(posed)):
        posed[i, 10:14] = boxset.quat_mul(rot, tuple(local[i, 10:14]))
    posed = posed.astype(f32)
    ref = host.query_sweep_box(load_scene("cube"), local.astype(f32), ALL)
    for ex in (False, True):
        out = (host.query_sweep_box_exhaustive if ex else host.query_sweep_box)(sc, posed, ALL)
        for i, (r, t, axes, nrm) in enumerate(cases):
            dl = float(np.linalg.norm(r[3:6]))
            if t is not None and np.isfinite(t) and cases[i][2] != {-1}:
                tol = host.sweep_box_bound(8.0, 2 * (8.0 + float(np.linalg.norm(pos))), t * dl, 1.0) / dl
                assert abs(float(out["distance"][i]) - float(ref["distance"][i])) <= 2 * tol, (ex, i, float(out["distance"][i]), float(ref["distance"][i]), tol)
                if nrm is not None and t > 0:
                    assert np.allclose(out["normal"][i], m[:3, :3] @ np.array(nrm), atol=1e-5), (ex, i)
            elif t is not None:
                assert np.isinf(out["distance"][i]) == np.isinf(ref["distance"][i])


def test_analytic_sphere_and_plane(host):
    hot = load_scene("cube").blas[0].tri_hot
    tris = np.stack([hot["position_0"], hot["position_0"] + hot["position_edge_1"], hot["position_0"] + hot["position_edge_2"]], axis=1)
    sc = hitset.mesh_scene([tris], spheres=[((6.0, 0.0, 0.0), 2.0), ((0.0, 0.0, 40.0), 10.0)], planes=[((0.0, 1.0, 0.0), 5.0)])        # the plane y = -5
    q = tuple(np.array([1.0, 2.0, 3.0, 4.0]) / np.sqrt(30.0))
    r3 = np.sqrt(3.0)
    cases = [
        (bs.row((6.0, 0.0, 6.0), (0.0, 0.0, -1.0), 20.0, (0.5, 0.5, 0.5)), 3.5, 14, 1, (0.0, 0.0, 1.0)),               # a face onto the shell from outside
        (bs.row((6.0, 0.0, 6.0), (0.0, 0.0, -2.0), 20.0, (0.25, 0.25, 0.5)), 1.75, 14, 1, (0.0, 0.0, 1.0)),
        (bs.row((11.0, 5.0, 5.0), (-1.0, -1.0, -1.0), 20.0, (1.0, 1.0, 1.0)), 4.0 - 2.0 / r3, 14, 1, (1 / r3, 1 / r3, 1 / r3)),      # a corner along the diagonal
        (bs.row((0.0, 0.0, 40.0), (0.0, 0.0, 1.0), 50.0, (1.0, 1.0, 1.0)), np.sqrt(98.0) - 1.0, 14, 2, (0.1, 0.1, -np.sqrt(0.98))),      # from inside: four far corners reach the shell together; the one at (-1, -1, +1) is reported
        (bs.row((0.0, 0.0, 40.0), (1.0, 0.0, 0.0), 50.0, (0.0, 0.0, 0.0)), 10.0, 14, 2, (-1.0, 0.0, 0.0)),                     # a point from the centre
        (bs.row((6.0, 0.0, 2.0), (0.0, 1.0, 0.0), 20.0, (0.5, 0.5, 0.5), q), 0.0, 13, 1, (0.0, 0.0, 0.0)),                     # across the shell
        (bs.row((6.0, 0.0, 6.0), (0.0, 0.0, 1.0), 20.0, (0.5, 0.5, 0.5)), np.inf, -1, -1, (0.0, 0.0, 0.0)),                    # away from it
        (bs.row((6.0, 3.0, 6.0), (0.0, 0.0, -1.0), 20.0, (0.5, 0.5, 0.5)), np.inf, -1, -1, (0.0, 0.0, 0.0)),                   # past it: the box's edge clears the ball by 0.5
        (bs.row((3.0, -3.0, 3.0), (0.0, -1.0, 0.0), 20.0, (0.25, 0.5, 0.25)), 1.5, 15, 3, (0.0, 1.0, 0.0)),                    # onto the plane
        (bs.row((3.0, -8.0, 3.0), (0.0, 2.0, 0.0), 20.0, (0.25, 0.5, 0.25)), 1.25, 15, 3, (0.0, -1.0, 0.0)),                   # from below
        (bs.row((3.0, -3.0, 3.0), (1.0, 1.0, 0.0), 20.0, (0.25, 0.5, 0.25)), np.inf, -1, -1, (0.0, 0.0, 0.0)),                 # receding
        (bs.row((3.0, -3.0, 3.0), (1.0, 0.0, 0.0), np.inf, (0.25, 0.5, 0.25)), np.inf, -1, -1, (0.0, 0.0, 0.0)),               # along it
        (bs.row((3.0, -4.5, 3.0), (1.0, 0.0, 0.0), 20.0, (0.25, 0.5, 0.25)), 0.0, 13, 3, (0.0, 0.0, 0.0)),                     # standing on it
    ]
    rows = np.stack([c[0] for c in cases])
    for ex in (False, True):
        out = (host.query_sweep_box_exhaustive if ex else host.query_sweep_box)(sc, rows, ALL)
        for i, (r, t, axis, obj, nrm) in enumerate(cases):
            if np.isinf(t):
                assert np.isinf(out["distance"][i]), (ex, i, float(out["distance"][i]))
            else:
                assert abs(float(out["distance"][i]) - t) <= 64 * U * (60.0 + t), (ex, i, float(out["distance"][i]), t)
            assert out["axis"][i] == axis and out["object_id"][i] == obj and out["triangle_id"][i] == -1, (ex, i, int(out["axis"][i]), int(out["object_id"][i]))
            assert np.allclose(out["normal"][i], nrm, atol=1e-5), (ex, i, out["normal"][i], nrm)


# ---- 6. against the merged queries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "materials_aniso"])
def test_point_box_against_query_closest(host, name):
    """A point box is a ray.  The host has no twin of query_closest; its closest hit is host.query_hits with max_hits = 1, the same hit test.
    Compared per row, on triangle answers both name, where the returned normal is within COS_FLOOR of the motion and the bound does not
    exclude the contact: |t_box - t_ray| |d| <= sweep_box_bound(S, W, T, kappa of the winning axis) / cos + the hit test's own margin in
    t, S, W and kappa the row's own at its contact."""
    sc, rows, lab, w, e = row_set(host, name)
    pts = rows[~bs.is_dead(rows)].copy(); pts[:, 7:10] = 0.0; pts[:, 6] = np.inf
    out = host.query_sweep_box(sc, pts, ALL)
    segs = np.ascontiguousarray(np.concatenate([pts[:, :6], np.full((len(pts), 1), np.inf, f32)], axis=1))
    hits = host.query_hits(sc, segs, 1, ("distance", "object_id", "triangle_id"), count=False)
    cl = hits["distance"][:, 0]
    dl = np.linalg.norm(pts[:, 3:6].astype(np.float64), axis=1)
    ni = len(sc.instances)
    compared, worst, skipped = 0, 0.0, 0
    for i in np.flatnonzero(np.isfinite(out["distance"]) & np.isfinite(cl) & (out["distance"] > 0) & (out["object_id"] < ni) & (hits["object_id"][:, 0] < ni)):
        t = float(out["distance"][i])
        S, W, kap, k, cos, excluded, sliver, gap = bs.contact(sc, pts[i], t, int(out["object_id"][i]), int(out["triangle_id"][i]), out["normal"][i])
        if excluded or cos < bs.COS_FLOOR or sliver > 4:
            skipped += 1; continue
        S0 = bs.contact(sc, pts[i], 0.0, int(out["object_id"][i]), int(out["triangle_id"][i]), out["normal"][i])[0]      # |o - p0| + |e1| + |e2|: the hit test's scale
        bound = host.sweep_box_bound(S, W, t * dl[i], kap) / cos + host.hits_margin(sliver / cos, (S0 + 8 * W) / dl[i]) * dl[i]
        err = abs(t - float(cl[i])) * dl[i]
        worst = max(worst, err / bound); compared += 1
        assert err <= bound, (name, i, t, float(cl[i]), err, bound, k, kap, cos)
    one_sided = np.isfinite(out["distance"]) != np.isfinite(cl)
    print(f"{name}: {compared} rays compared, worst {worst:.3g} of its bound, {skipped} skipped, {int(one_sided.sum())} answered by one only")
    assert compared > len(pts) // 4
    assert one_sided.sum() * 20 <= len(pts)


@pytest.mark.parametrize("name", SCENES)
def test_t_zero_rows_against_query_overlap(host, name):
    sc, rows, lab, w, e = row_set(host, name)
    zero = np.flatnonzero(w["distance"] == 0)
    assert len(zero) >= 10
    boxes = bs.box_of(rows[zero])
    ex = host.query_overlap(sc, boxes, 8, exhaustive=True)
    first = host.query_overlap(sc, boxes, 1)
    from test_query_overlap_cpu import fp64_expectation
    clear = np.array([x[2] for x in fp64_expectation(host, sc, boxes)]) if name != "monkey_small" else np.zeros(len(zero), bool)      # every pair decided by the margin
    clear &= np.array([not (0 <= w["object_id"][i] < len(sc.instances) and has_splits(sc, int(w["object_id"][i]))) for i in zero])      # and no split leaves: there the two walks may name different slots
    for j, i in enumerate(zero):
        pair = (int(w["object_id"][i]), int(w["triangle_id"][i]))
        assert w["axis"][i] == 13, (name, i, int(w["axis"][i]))
        listed = list(zip(ex["object_id"][j].tolist(), ex["triangle_id"][j].tolist()))
        assert pair in listed[:int(min(ex["count"][j], 8))] or ex["count"][j] > 8, (name, i, pair, listed)
        if clear[j]:
            assert pair == (int(first["object_id"][j, 0]), int(first["triangle_id"][j, 0])), (name, i, pair)
    assert name == "monkey_small" or clear.sum() >= 5
    never = np.flatnonzero((w["distance"] > 0) & ~bs.is_dead(rows))
    assert not host.query_overlapped(sc, bs.box_of(rows[never]), exhaustive=True).any(), "a row that overlaps where it starts answers t > 0"


@pytest.mark.parametrize("name", ["cube", "materials_aniso"])
def test_cubes_between_the_two_balls_of_query_sweep(host, name):
    """A cube of half extent h lies between its inscribed ball (h) and its circumscribed ball (sqrt(3) h): t_outer <= t_box <= t_inner, each
    within both queries' bounds.  Per row: the box's bound at its own contact (S, W, kappa of its winning axis), the ball's sweep_bound at
    the ball's contact (S = the distance to its contact point + the mesh's longest edge twice, its r), both divided by |d| cos of their own
    contact normal; rows where either normal is beyond COS_FLOOR of the motion, or the box's contact is one its bound excludes, are skipped."""
    sc, rows, lab, w, e = row_set(host, name)
    cubes = rows[~bs.is_dead(rows) & bs.in_classes(lab, ("approach", "face_on", "vertex_face", "d_inf", "edge_edge"))].copy()
    cubes[:, 7:10] = cubes[:, 7:8]; cubes[:, 6] = np.inf
    cubes = cubes[cubes[:, 7] > 0]
    box = host.query_sweep_box(sc, cubes, ALL)
    tb = box["distance"]
    ni = len(sc.instances)
    emax = max(float(max(np.linalg.norm(b.tri_hot["position_edge_1"], axis=1).max(), np.linalg.norm(b.tri_hot["position_edge_2"], axis=1).max(),
                         np.linalg.norm(b.tri_hot["position_edge_2"] - b.tri_hot["position_edge_1"], axis=1).max())) for b in sc.blas)
    dl = np.linalg.norm(cubes[:, 3:6].astype(np.float64), axis=1)

    def ball(radius):
        sw = np.ascontiguousarray(np.concatenate([cubes[:, :7], radius[:, None]], axis=1).astype(f32))
        o = host.query_sweep(sc, sw, ("distance", "position"))
        slack = np.full(len(sw), np.nan)
        for i in np.flatnonzero(np.isfinite(o["distance"]) & (o["distance"] > 0)):
            c = sw[i, :3].astype(np.float64) + float(o["distance"][i]) * sw[i, 3:6].astype(np.float64)
            n = c - o["position"][i].astype(np.float64)
            cos = abs(float(n @ sw[i, 3:6])) / (float(np.linalg.norm(n)) * dl[i]) if np.linalg.norm(n) > 0 else 0.0
            if cos >= bs.COS_FLOOR:
                slack[i] = host.sweep_bound(float(radius[i]) + 2 * emax, bs.world_scale(sc, c), float(o["distance"][i]) * dl[i], float(radius[i])) / (cos * dl[i])
        return o["distance"], slack
    (outer, so), (inner, si) = ball(cubes[:, 7] * f32(np.sqrt(3.0))), ball(cubes[:, 7].copy())
    lower = upper = 0
    for i in np.flatnonzero(np.isfinite(tb) & (tb > 0) & (box["object_id"] >= 0) & (box["object_id"] < ni)):
        t = float(tb[i])
        S, W, kap, k, cos, excluded, _, _ = bs.contact(sc, cubes[i], t, int(box["object_id"][i]), int(box["triangle_id"][i]), box["normal"][i])
        if excluded or cos < bs.COS_FLOOR:
            continue
        sb = host.sweep_box_bound(S, W, t * dl[i], kap) / (cos * dl[i])
        if np.isfinite(so[i]):
            assert outer[i] <= t + sb + so[i], (name, i, float(outer[i]), t, sb, so[i]); lower += 1
        if np.isfinite(si[i]):
            assert t <= inner[i] + sb + si[i], (name, i, t, float(inner[i]), sb, si[i]); upper += 1
    print(f"{name}: {len(cubes)} cubes, {lower} compared with the circumscribed ball, {upper} with the inscribed")
    assert len(cubes) >= 40 and lower >= 20 and upper >= 20
    assert (outer < tb).sum() > len(cubes) // 4 and (tb < inner).sum() > len(cubes) // 4


# ---- 7. masks, two trees, the stack ---------------------------------------------------------------------------------------------------------
def test_masks(host):
    sc, rows, lab, w, e = row_set(host, "coincident")
    n = len(rows)
    M = len(sc.instances) + len(sc.spheres) + len(sc.planes)
    ones = np.full(M, 0xFFFFFFFF, np.uint32)
    for kw in ({"mask": 0xFFFFFFFF}, {"object_masks": ones}, {"mask": np.full(n, -1, np.int32), "object_masks": ones}):
        f = host.query_sweep_box(sc, rows, ALL, **kw)
        assert all(np.array_equal(f[k], w[k]) for k in ALL), kw
    z = host.query_sweep_box(sc, rows, ALL, mask=0)
    assert np.isinf(z["distance"]).all() and (z["object_id"] == -1).all() and (z["axis"] == -1).all() and z["stack_max"] == 0
    om = (1 << (np.arange(M) % 4)).astype(np.uint32)
    rm = np.array([(1, 2, 4, 8, 3, 12, 15, 0)[i % 8] for i in range(n)], np.uint32)
    f = host.query_sweep_box(sc, rows, ALL, mask=rm, object_masks=om)
    fe = host.query_sweep_box_exhaustive(sc, rows, ALL, mask=rm, object_masks=om)
    assert not (f["distance"] < fe["distance"]).any() and (f["distance"] >= w["distance"]).all() and (f["distance"] > w["distance"]).any()
    same = f["distance"] == fe["distance"]
    assert same.sum() * 50 >= 49 * n and all(np.array_equal(f[k][same], fe[k][same]) for k in ALL)
    for out in (f, fe):
        ids = out["object_id"]
        assert ((om[ids[ids >= 0]] & rm[ids >= 0]) != 0).all(), "a hidden object answers"
        assert np.isinf(out["distance"][rm == 0]).all()
    # the exhaustive search over the visible set alone: the same scene with the hidden instances' rows answered under a mask of one object each
    for i in np.flatnonzero(np.isfinite(f["distance"]))[:40]:
        one = np.zeros(M, np.uint32); one[int(f["object_id"][i])] = 1
        alone = host.query_sweep_box(sc, rows[i:i + 1], ALL, mask=1, object_masks=one)
        assert all(np.array_equal(alone[k][0], f[k][i]) for k in ALL), i
    # coincident instances 0 and 1 with different masks: the row's mask chooses which of the two answers, with the same slot and t
    a = host.query_sweep_box(sc, rows, ALL, mask=1, object_masks=om)
    b = host.query_sweep_box(sc, rows, ALL, mask=2, object_masks=om)
    both = (a["object_id"] == 0) & (b["object_id"] == 1)
    assert both.sum() > 20 and np.array_equal(a["distance"][both], b["distance"][both]) and np.array_equal(a["triangle_id"][both], b["triangle_id"][both]) and not (a["object_id"] == 1).any()


def test_two_trees_over_the_same_triangles(host):
    """The cube's mesh under its own BVH and under a chain over the same slots: the same answers."""
    import copy
    from pyrtx import scene_io as sio
    sc = load_scene("cube")
    rows = row_set(host, "cube")[1]
    hot = sc.blas[0].tri_hot
    n = len(hot)
    nodes = np.zeros(2 * n - 1, sio.BVH_NODE)
    box = lambda t: np.stack([hot["position_0"][t], hot["position_0"][t] + hot["position_edge_1"][t], hot["position_0"][t] + hot["position_edge_2"][t]])
    k = 0
    for d in range(n - 1):                                                  # node k = (leaf d, the rest) at (2d + 1, 2d + 2)
        nodes[k]["left_or_first"] = 2 * d + 1; nodes[k]["count"] = np.uint32(1 << 30).astype(np.int32)
        nodes[2 * d + 1]["left_or_first"] = d; nodes[2 * d + 1]["count"] = 1
        nodes[2 * d + 1]["aabb_min"] = box(d).min(axis=0); nodes[2 * d + 1]["aabb_max"] = box(d).max(axis=0)
        k = 2 * d + 2
    nodes[k]["left_or_first"] = n - 1; nodes[k]["count"] = 1; nodes[k]["aabb_min"] = box(n - 1).min(axis=0); nodes[k]["aabb_max"] = box(n - 1).max(axis=0)
    for d in range(n - 2, -1, -1):
        kk = 0 if d == 0 else 2 * d
        nodes[kk]["aabb_min"] = np.minimum(nodes[2 * d + 1]["aabb_min"], nodes[2 * d + 2]["aabb_min"]); nodes[kk]["aabb_max"] = np.maximum(nodes[2 * d + 1]["aabb_max"], nodes[2 * d + 2]["aabb_max"])
    other = copy.deepcopy(sc)
    other.blas[0] = sio.Blas(nodes, hot, sc.blas[0].tri_cold, sc.blas[0].material_offset, n)
    a, b = host.query_sweep_box(sc, rows, ALL), host.query_sweep_box(other, rows, ALL)
    assert all(np.array_equal(a[k], b[k]) for k in ALL)
    assert b["stack_max"] > a["stack_max"] and a["stack_max"] <= stack_need(sc) and b["stack_max"] <= stack_need(other), (a["stack_max"], b["stack_max"], stack_need(other))
