"""rtx_set_blas_topology / rtx_blas_vertex_normals on the GPU: smooth vertex normals from positions and indices in device memory, on the
context's stream, into a device buffer that rtx_refit_blas and rtx_build_blas take as it is.

What is compared with what (all bit for bit; nothing here is a tolerance):
  parity        Renderer.vertex_normals  ==  host.vertex_normals (rtxh_vertex_normals: the same header as a scatter loop on the CPU,
                tests/test_vertex_normals_cpu.py) on the shapes that cross the kernels' edges, the golden meshes, the rule cases and the
                hostile floats, with unaligned views and a guard row behind the output;
  reproducible  the same call twice, and the triangles in reversed order against the twin for that order;
  mesh path     refit_blas(i, pos, vertex_normals(i, pos)) and alloc_blas / build_blas with the computed normals: read_blas against the host
                twins, frames against the oracle;
  ordering      topology -> normals -> refit -> render on a torch stream with nothing synchronised in between;
  errors        every status code in the documented order, the frame unchanged after each.
"""
import numpy as np
import pytest

import normalset as ns
import util
from test_gpu_parity import MODES
from test_tlas_balanced_cpu import poses
from test_blas_refit_cpu import FRAME_CASES, build, deform, tori_scene
from test_gpu_blas_refit import assert_same_blas, assert_same_frame, dev
from test_gpu_blas_build import small
from test_blas_build_cpu import twin

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, LIMIT, STATE = 1, 4, 5
PATTERN = 0x5ca1ab1e


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


_scene = {}


def cube_renderer(api):
    """A small context with one uploaded BLAS under id 0: the topology's counts need not be the BLAS's own."""
    if "cube" not in _scene:
        _scene["cube"] = util.load_golden("cube")[0]
    return api.Renderer(_scene["cube"])


def shared_renderer(api):
    """One context for all parity cases: every case with other counts allocates anew under the same id."""
    if "renderer" not in _scene:
        _scene["renderer"] = cube_renderer(api)
    return _scene["renderer"]


def offset_view(a, dtype):
    """The array as a device tensor that starts 4 bytes into its allocation, with one guard row of PATTERN behind it -> (view, whole)"""
    import torch
    a = np.ascontiguousarray(a, dtype)
    flat = torch.full((1 + a.size + 3,), PATTERN, dtype=torch.int32, device="cuda")
    view = flat[1:1 + a.size].view(torch.float32 if dtype == f32 else torch.int32).view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4
    return view, flat


def device_normals(r, pos, idx, blas_id=0, unaligned=False):
    """Topology and normals through the Renderer, the output in a (V + 1, 3) allocation whose last row is a guard -> (V, 3) float32"""
    import torch
    V = len(pos)
    if unaligned:
        p, keep_p = offset_view(pos, f32)
        i, keep_i = offset_view(idx, np.int32)
        o, keep_o = offset_view(np.zeros((V, 3), f32), f32)
        guard = keep_o[1 + 3 * V:]
    else:
        p, i = dev(pos), dev(idx, np.int32)
        whole = torch.full((V + 1, 3), PATTERN, dtype=torch.int32, device="cuda").view(torch.float32)
        o, guard = whole[:V], whole[V:].view(torch.int32)
    torch.cuda.synchronize()                                        # torch filled the tensors on its own stream
    r.set_blas_topology(blas_id, i, V)
    assert r.vertex_normals(blas_id, p, o) is o
    r.synchronize()
    assert bool((guard == PATTERN).all()), "memory behind the output was written"
    return o.cpu().numpy()


def same(a, b):
    return np.ascontiguousarray(a, f32).tobytes() == np.ascontiguousarray(b, f32).tobytes()


def parity_cases():
    cases = dict(ns.shapes())
    for m in ("icosphere", "Torus", "Monkey"):
        cases[m] = ns.indexed(m)
    for name, (pos, idx, _, _) in ns.rule_cases().items():
        cases["rule_" + name] = (pos, idx)
    for k, (pos, idx, _) in enumerate(ns.hostile_cases()):
        cases[f"hostile{k}"] = (pos, idx)
    pos, idx = ns.indexed("icosphere")
    for e in (-60, 40):
        cases[f"scale{e}"] = (np.ldexp(pos, e).astype(f32), idx)
    return cases


CASES = parity_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_the_host_twin(api, name):
    from pyrtx import host
    pos, idx = CASES[name]
    want = host.vertex_normals(pos, idx)
    got = device_normals(shared_renderer(api), pos, idx)
    assert same(got, want), name
    assert np.isfinite(got).all()
    if name == "Monkey":
        assert ns.is_zero(got).sum() == 1
    if name in ("V1", "rule_all_invalid"):
        assert ns.is_zero(got).all()


@pytest.mark.parametrize("name", ["T86", "V257", "fan257", "Torus", "rule_padded", "hostile8"])
def test_unaligned_views(api, name):
    """positions, indices and out start 4 bytes into their allocations: not 16-byte aligned."""
    from pyrtx import host
    pos, idx = CASES[name]
    assert same(device_normals(shared_renderer(api), pos, idx, unaligned=True), host.vertex_normals(pos, idx)), name


def test_reproducible_and_order_of_triangles(api):
    import torch
    from pyrtx import host
    pos, idx = ns.indexed("Monkey")
    r = cube_renderer(api)
    p, i, back = dev(pos), dev(idx, np.int32), dev(idx[::-1], np.int32)
    torch.cuda.synchronize()
    r.set_blas_topology(0, i, len(pos))
    a = r.vertex_normals(0, p)
    r.synchronize(); first = a.cpu().numpy()
    b = r.vertex_normals(0, p)
    assert b is a, "the renderer's own tensor is made once per id"
    r.synchronize(); second = b.cpu().numpy()
    assert first.tobytes() == second.tobytes() == host.vertex_normals(pos, idx).tobytes()
    r.set_blas_topology(0, back, len(pos))                          # the same counts: no alloc, the index is rebuilt
    c = torch.empty_like(p)
    r.vertex_normals(0, p, c)
    r.synchronize()
    want = host.vertex_normals(pos, idx[::-1])
    assert c.cpu().numpy().tobytes() == want.tobytes()
    assert want.tobytes() != first.tobytes(), "the order of the additions shows in the last bits"
    r.set_blas_topology(0, i[:100], len(pos))                       # other counts: a new alloc under the same id
    r.vertex_normals(0, p, c)
    r.synchronize()
    assert c.cpu().numpy().tobytes() == host.vertex_normals(pos, idx[:100]).tobytes()


# ---- through the mesh path ------------------------------------------------------------------------------------------------------------------
_torus = {}


def torus():
    """-> (SBVH Blas of the Torus soup, slot vertices into the OBJ's `v` lines, positions (V, 3), faces (T, 3), (uv, material ids) of the soup)"""
    from pyrtx import host
    if not _torus:
        blas, soup_pos, _, uv, mid = build("Torus", reference_sbvh=True)
        pos, faces = ns.indexed("Torus")
        assert util.bit_exact(pos[faces], soup_pos.reshape(-1, 3, 3)), "the loader keeps the file's triangle order"
        _torus["case"] = (blas, host.slot_vertices(blas, faces), pos, faces, (uv, mid))
    return _torus["case"]


_oracle = {}


def oracle_frame(sc, key):
    import orc
    if key not in _oracle:
        _oracle[key] = orc.OracleScene(sc).render(threads=8)
    return _oracle[key]


@pytest.mark.parametrize("kind,seed,amp", FRAME_CASES[:2])
def test_refit_with_computed_normals(api, kind, seed, amp):
    """The step is refit_blas(i, pos, vertex_normals(i, pos)): the BLAS equals the refit twin given the normals twin's output, the frame the
    oracle's of a mesh freshly built from the deformed positions and those normals."""
    import torch
    from pyrtx import host
    blas, sv, pos, faces, (uv, mid) = torus()
    verts = deform(pos, kind, seed, amp)
    normals = host.vertex_normals(verts, faces)
    want = host.blas_refit(blas, sv, verts, normals)
    fresh = host.build_blas(verts[faces], normals[faces], uv, mid, 0, reference_sbvh=True)
    sc, tw, fr = small(tori_scene(blas)), small(tori_scene(want)), small(tori_scene(fresh))
    ref = oracle_frame(fr, (kind, "fresh"))
    assert_same_frame(oracle_frame(tw, (kind, "refit")), ref, "the oracle's frames of the refitted and the freshly built tree")
    r = api.Renderer(sc)
    r.bind_blas_vertices(0, sv, len(verts))
    p_, q_ = poses("tori16", 1)
    v, f, p, q = dev(verts), dev(faces, np.int32), dev(p_), dev(q_)
    torch.cuda.synchronize()
    r.set_blas_topology(0, f, len(verts))
    r.refit_blas(0, v, r.vertex_normals(0, v))
    r.update_instances(p, q)
    assert_same_blas(r.read_blas(0), want, kind)
    assert want.tri_cold.tobytes() != host.blas_refit(blas, sv, verts).tri_cold.tobytes(), "the normals moved"
    for mode in ("default", "serial_lane"):
        assert_same_frame(r.render(**MODES[mode]), ref, f"{kind}, {mode}")
    assert not np.array_equal(ref["packed"], oracle_frame(sc, "base")["packed"])


def test_build_with_computed_normals(api):
    """alloc_blas / build_blas over the Torus padded with invalid triangles, its normals computed from the same padded index buffer."""
    import torch
    from pyrtx import host
    blas, _, pos, faces, _ = torus()
    verts = deform(pos, "wave", 2, 1.0)
    idx = ns.padded(faces, len(verts))
    normals = host.vertex_normals(verts, idx)
    assert same(normals, host.vertex_normals(verts, faces))
    want, sv, order = twin(verts, idx, normals)
    tw = small(tori_scene(want))
    r = api.Renderer(small(tori_scene(blas)))
    r.alloc_blas(0, len(idx), len(verts))
    p_, q_ = poses("tori16", 1)
    v, f, p, q = dev(verts), dev(idx, np.int32), dev(p_), dev(q_)
    torch.cuda.synchronize()
    r.set_blas_topology(0, f, len(verts))
    r.build_blas(0, v, f, r.vertex_normals(0, v))
    r.update_instances(p, q)
    assert_same_blas(r.read_blas(0), want, "after the build")
    ref = oracle_frame(tw, "built")
    for mode in ("default", "serial_lane"):
        assert_same_frame(r.render(**MODES[mode]), ref, mode)


def test_stream_order(api):
    """On a torch stream of its own: topology -> normals -> refit -> update -> render with nothing synchronised in between equals the
    synchronised sequence; a second vertex_normals into the same tensor after new positions gives the new normals."""
    import torch
    from pyrtx import host
    blas, sv, pos, faces, _ = torus()
    va, vb = deform(pos, *FRAME_CASES[0]), deform(pos, *FRAME_CASES[1])
    sc = small(tori_scene(blas))
    p_, q_ = poses("tori16", 1)
    frames = []
    for own_stream in (False, True):
        r = api.Renderer(sc)
        r.bind_blas_vertices(0, sv, len(pos))
        a, b, f, p, q = dev(va), dev(vb), dev(faces, np.int32), dev(p_), dev(q_)
        out = torch.zeros_like(a)
        r.set_views(np.concatenate([sc.camera, sc.camera]))
        torch.cuda.synchronize()
        if own_stream:
            s = torch.cuda.Stream()
            r.set_stream(s.cuda_stream)
        for view, v in enumerate((a, b)):
            r.set_blas_topology(0, f, len(pos))
            assert r.vertex_normals(0, v, out) is out
            r.refit_blas(0, v, out)
            r.update_instances(p, q)
            r.render_views_async(view, 1)
            if not own_stream:
                r.synchronize()
        rgb, packed = r.read_views(0, 2)
        r.synchronize()
        assert out.cpu().numpy().tobytes() == host.vertex_normals(vb, faces).tobytes()
        assert_same_blas(r.read_blas(0), host.blas_refit(blas, sv, vb, host.vertex_normals(vb, faces)), f"own stream {own_stream}")
        frames.append((rgb, packed))
        if own_stream:
            r.set_stream(None)
    assert util.bit_exact(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1])
    assert not np.array_equal(frames[0][1][0], frames[0][1][1]), "the two deformations differ"
    for view, (v, kind) in enumerate(((va, "a"), (vb, "b"))):
        tw = small(tori_scene(host.blas_refit(blas, sv, v, host.vertex_normals(v, faces))))
        ref = oracle_frame(tw, ("stream", kind))
        assert util.bit_exact(frames[1][0][view], ref["rgb"]) and np.array_equal(frames[1][1][view], ref["packed"]), view


def test_errors(api):
    import torch
    from pyrtx import host
    pos, idx = ns.indexed("icosphere")
    T, V = len(idx), len(pos)
    p, i = dev(pos), dev(idx, np.int32)
    out = torch.full((V, 3), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r = cube_renderer(api)
    lib, ctx = r.lib, r.ctx
    base = r.render()
    # rtx_alloc_blas_topology: 1. arguments  2. limit  3. state
    assert lib.rtx_alloc_blas_topology(ctx, -1, T, V) == INVALID
    assert lib.rtx_alloc_blas_topology(ctx, 1 << 20, T, V) == INVALID
    assert lib.rtx_alloc_blas_topology(ctx, 7, 0, V) == INVALID                                      # the counts come before the unknown id
    assert lib.rtx_alloc_blas_topology(ctx, 7, T, 0) == INVALID
    assert lib.rtx_alloc_blas_topology(ctx, 7, (1 << 28) + 1, V) == LIMIT                            # the limit comes before the unknown id
    assert lib.rtx_alloc_blas_topology(ctx, 7, T, V) == STATE
    # the other two before any alloc: 1. pointers  2. state
    assert lib.rtx_set_blas_topology(ctx, 7, None) == INVALID
    assert lib.rtx_set_blas_topology(ctx, 0, i.data_ptr() + 2) == INVALID
    assert lib.rtx_set_blas_topology(ctx, 7, i.data_ptr()) == STATE
    assert lib.rtx_set_blas_topology(ctx, -1, i.data_ptr()) == STATE
    assert lib.rtx_set_blas_topology(ctx, 0, i.data_ptr()) == STATE                                  # uploaded, no topology allocated
    assert lib.rtx_blas_vertex_normals(ctx, 7, None, out.data_ptr()) == INVALID
    assert lib.rtx_blas_vertex_normals(ctx, 7, p.data_ptr(), None) == INVALID
    assert lib.rtx_blas_vertex_normals(ctx, 0, p.data_ptr() + 1, out.data_ptr()) == INVALID
    assert lib.rtx_blas_vertex_normals(ctx, 0, p.data_ptr(), out.data_ptr() + 2) == INVALID
    assert lib.rtx_blas_vertex_normals(ctx, 7, p.data_ptr(), out.data_ptr()) == STATE
    assert lib.rtx_blas_vertex_normals(ctx, 0, p.data_ptr(), out.data_ptr()) == STATE
    assert lib.rtx_alloc_blas_topology(ctx, 0, T, V) == 0
    assert lib.rtx_blas_vertex_normals(ctx, 0, p.data_ptr(), out.data_ptr()) == STATE                # allocated, no topology set
    assert lib.rtx_blas_vertex_normals(ctx, 0, None, out.data_ptr()) == INVALID
    r.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote the output"
    assert_same_frame(r.render(), base, "after refused calls")
    assert lib.rtx_set_blas_topology(ctx, 0, i.data_ptr()) == 0
    assert lib.rtx_blas_vertex_normals(ctx, 0, p.data_ptr(), out.data_ptr()) == 0
    r.synchronize()
    want = host.vertex_normals(pos, idx)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    # a refused alloc leaves the state it was to replace
    assert lib.rtx_alloc_blas_topology(ctx, 0, 0, V) == INVALID
    assert lib.rtx_alloc_blas_topology(ctx, 0, (1 << 28) + 1, V) == LIMIT
    assert lib.rtx_set_blas_topology(ctx, 0, None) == INVALID
    out.fill_(7.0); torch.cuda.synchronize()
    assert lib.rtx_blas_vertex_normals(ctx, 0, p.data_ptr(), out.data_ptr()) == 0
    r.synchronize()
    assert out.cpu().numpy().tobytes() == want.tobytes()
    # a new alloc forgets the topology that was set
    assert lib.rtx_alloc_blas_topology(ctx, 0, T, V) == 0
    assert lib.rtx_blas_vertex_normals(ctx, 0, p.data_ptr(), out.data_ptr()) == STATE
    assert lib.rtx_set_blas_topology(ctx, 0, i.data_ptr()) == 0
    # Python-side checks
    with pytest.raises(TypeError):
        r.set_blas_topology(0, i.long(), V)
    with pytest.raises(ValueError):
        r.set_blas_topology(0, i.cpu(), V)
    with pytest.raises(TypeError):
        r.vertex_normals(0, p.double())
    with pytest.raises(ValueError):
        r.vertex_normals(0, p, out[:-1])
    with pytest.raises(api.RtxError):
        r.set_blas_topology(7, i, V)
    assert_same_frame(r.render(), base, "after the errors")
    # uploading the id again drops the topology
    r.upload_scene(_scene["cube"])
    assert lib.rtx_blas_vertex_normals(ctx, 0, p.data_ptr(), out.data_ptr()) == STATE
    assert lib.rtx_set_blas_topology(ctx, 0, i.data_ptr()) == STATE
    r._topology_shapes = {0: (T, V)}                                                                  # the Renderer's record is stale: it allocates again
    r.set_blas_topology(0, i, V)
    got = r.vertex_normals(0, p)
    r.synchronize()
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert_same_frame(r.render(), base, "at the end")


def test_two_contexts_do_not_mix(api):
    import torch
    from pyrtx import host
    pa, ia = ns.indexed("icosphere")
    pb, ib = ns.indexed("Torus")
    ra, rb = cube_renderer(api), cube_renderer(api)
    a, b = (dev(pa), dev(ia, np.int32)), (dev(pb), dev(ib, np.int32))
    torch.cuda.synchronize()
    ra.set_blas_topology(0, a[1], len(pa)); rb.set_blas_topology(0, b[1], len(pb))
    na, nb = ra.vertex_normals(0, a[0]), rb.vertex_normals(0, b[0])
    ra.synchronize(); rb.synchronize()
    assert na.cpu().numpy().tobytes() == host.vertex_normals(pa, ia).tobytes()
    assert nb.cpu().numpy().tobytes() == host.vertex_normals(pb, ib).tobytes()
    with pytest.raises(ValueError):
        ra.vertex_normals(0, b[0])                                  # the other context's vertex count
