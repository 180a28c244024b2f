"""rtx_update_instances on the GPU: poses in device memory -> instance records, world AABBs and the balanced TLAS, on the context's stream.

What is compared with what (all bit for bit; nothing here is a tolerance):
  records   read_frame_state() after the device update  ==  rtxh_scene_update's rtx_instance records (the host path of today) and
            rtxh_tlas_build_balanced's nodes / indices (the same builder on the CPU, tests/test_tlas_balanced_cpu.py), on the one-workgroup
            path and on the multi-launch path (RTX_UPDATE_SMALL_MAX=0 forces it on the same input);
  frames    a frame rendered after the device update  ==  the oracle given the read-back state, and  ==  a second context given the
            read-back state through plain rtx_set_frame, in every launch shape;
  ordering  render, update, render with nothing synchronised in between: each frame shows the poses it was queued with.
The hostile-pose test is a parity test on legal input (any float is a legal pose), like the NaN rays of tests/rayset.py; it is the last
test of the file.
"""
import os
import subprocess
import sys

if __name__ == "__main__":                      # the hostile-pose child process: the paths tests/conftest.py sets up, torch first as there
    _repo = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path[:0] = [_repo, os.path.join(_repo, "oracle"), os.path.join(_repo, "cpu-raytracer_amd")]
    import torch  # noqa: F401

import numpy as np
import pytest

import util
from test_gpu_parity import MODES
from test_tlas_balanced_cpu import check_tree, poses

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, LIMIT, STATE = 1, 4, 5


@pytest.fixture(scope="module")
def api():
    from pyrtx import api as a
    a.load_library()
    return a


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, f32)).cuda()


def host_state(sc, pos, rot):
    """(instances, balanced nodes, balanced indices) for the poses from librtx_host; the instance records are checked against
    rtxh_instance_update's — the records the host path of today (rtxh_scene_update) hands to rtx_set_frame."""
    from pyrtx import host
    inst, nodes, idx = host.scene_update_balanced(sc, pos, rot)
    for i in range(len(pos)):
        b = int(sc.instances["blas_id"][i]); root = sc.blas[b].nodes[0]
        one, _, _ = host.instance_update(pos[i], rot[i], root["aabb_min"], root["aabb_max"], b)
        assert one["blas_id"][0] == inst["blas_id"][i]
        assert util.bit_exact(one["world"][0], inst["world"][i]) and util.bit_exact(one["world_inv"][0], inst["world_inv"][i]), i
    return inst, nodes, idx


def with_state(sc, state):
    import copy
    s = copy.copy(sc)
    s.instances, s.tlas_nodes, s.tlas_indices = state
    return s


def many_scene(n, seed):
    """n seeded instances of the tori16 golden's mesh around its camera's view; the frame state it starts from is the host's."""
    from pyrtx import host
    sc, _ = util.load_golden("tori16")
    rng = np.random.default_rng(seed)
    pos = (rng.uniform(-1, 1, (n, 3)) * np.array([14.0, 6.0, 10.0]) + np.array([0.0, 4.0, 14.0])).astype(f32)
    q = rng.normal(size=(n, 4)); rot = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    sc.instances = np.zeros(n, util.sio.INSTANCE)                  # blas_id 0
    sc.instances, sc.tlas_nodes, sc.tlas_indices = host.scene_update_balanced(sc, pos, rot)
    return sc, pos, rot


def assert_state(got, want, what=""):
    for g, w, name in zip(got, want, ("instances", "tlas nodes", "tlas indices")):
        assert len(g) == len(w) and g.tobytes() == w.tobytes(), (what, name)


def assert_same_frame(out, ref, what=""):
    assert out["stats"] == ref["stats"], (what, out["stats"], ref["stats"])
    assert util.bit_exact(out["rgb"], ref["rgb"]), what
    assert np.array_equal(out["packed"], ref["packed"]), what


_oracle = {}


def oracle_frame(sc, state, key):
    import orc
    if key not in _oracle:
        _oracle[key] = orc.OracleScene(with_state(sc, state)).render(threads=8)
    return _oracle[key]


@pytest.mark.parametrize("path", ["one_workgroup", "multi_launch"])
@pytest.mark.parametrize("name", ["dynamic", "tori16"])
def test_records_equal_the_host_update(api, name, path, monkeypatch):
    if path == "multi_launch":
        monkeypatch.setenv("RTX_UPDATE_SMALL_MAX", "0")
    sc, _ = util.load_golden(name)
    r = api.Renderer(sc)
    assert_state(r.read_frame_state(), (sc.instances, sc.tlas_nodes, sc.tlas_indices), "after rtx_set_frame")
    for f in (1, 2, 3):
        pos, rot = poses(name, f)
        p, q = dev(pos), dev(rot)
        r.update_instances(p, q)
        got = r.read_frame_state()
        assert_state(got, host_state(sc, pos, rot), f"{name} frame {f} {path}")


@pytest.mark.parametrize("path", ["one_workgroup", "multi_launch"])
def test_records_of_a_thousand_instances(api, path, monkeypatch):
    if path == "multi_launch":
        monkeypatch.setenv("RTX_UPDATE_SMALL_MAX", "0")
    sc, pos, rot = many_scene(1000, 11)
    r = api.Renderer(sc)
    rng = np.random.default_rng(12)
    for step in range(2):
        pos = (pos + rng.uniform(-0.5, 0.5, pos.shape)).astype(f32)
        p, q = dev(pos), dev(rot)
        r.update_instances(p, q)
        assert_state(r.read_frame_state(), host_state(sc, pos, rot), f"step {step} {path}")


def test_multi_launch_path_beyond_one_workgroup(api):
    """1 500 and 5 000 instances: the sizes that cannot take the one-workgroup kernel (levels above 10 get a launch each)."""
    for n in (1500, 5000):
        sc, pos, rot = many_scene(n, n)
        r = api.Renderer(sc)
        pos = (pos * f32(1.01)).astype(f32)
        p, q = dev(pos), dev(rot)
        r.update_instances(p, q)
        assert_state(r.read_frame_state(), host_state(sc, pos, rot), f"n = {n}")


@pytest.mark.parametrize("mode", list(MODES))
def test_frame_after_update_equals_oracle_and_host_path(api, mode):
    sc, _ = util.load_golden("tori16")
    pos, rot = poses("tori16", 3)
    r = api.Renderer(sc)
    p, q = dev(pos), dev(rot)
    r.update_instances(p, q)
    out = r.render(**MODES[mode])
    state = r.read_frame_state()
    assert_state(state, host_state(sc, pos, rot))
    assert_same_frame(out, oracle_frame(sc, state, "tori16_f3"), f"oracle, {mode}")
    ref = api.Renderer(with_state(sc, state)).render(**MODES[mode])            # the host path: the read-back state through rtx_set_frame
    assert_same_frame(out, ref, f"second context, {mode}")


@pytest.mark.parametrize("path", ["one_workgroup", "multi_launch"])
def test_dynamic_golden_through_the_device_path(api, path, monkeypatch):
    """dynamic after three device updates is the reference's golden frame (the balanced tree changes no pixel of it: the CPU test shows
    that for the oracle)."""
    if path == "multi_launch":
        monkeypatch.setenv("RTX_UPDATE_SMALL_MAX", "0")
    sc, g = util.load_golden("dynamic")
    r = api.Renderer(sc)
    for f in (1, 2, 3):
        pos, rot = poses("dynamic", f)
        p, q = dev(pos), dev(rot)
        r.update_instances(p, q)
        out = r.render()
    cmp = util.compare_to_golden(out, g)
    assert cmp["stats_equal"] and cmp["max_abs"] == 0.0 and cmp["n_diff_pixels"] == 0 and cmp["packed_mismatch"] == 0, cmp


def test_views_and_rays_with_aovs_after_update(api):
    sc, _ = util.load_golden("tori16")
    pos, rot = poses("tori16", 3)
    r = api.Renderer(sc)
    p, q = dev(pos), dev(rot)
    r.update_instances(p, q)
    state = r.read_frame_state()
    ref = oracle_frame(sc, state, "tori16_f3")
    names = ("depth", "position", "normal", "object_id", "triangle_id")
    r2 = api.Renderer(with_state(sc, state))
    want = r2.render_aovs(names)
    cams = np.concatenate([sc.camera, sc.camera])
    r.set_views(cams)
    views = r.render_views(aovs=names)
    r.set_rays(np.stack([api.pinhole_rays(sc.camera, sc.width, sc.height)] * 2))
    rays = r.render_rays(aovs=names, serial=True)
    for out, what in ((views, "views"), (rays, "rays")):
        for v in range(2):
            assert util.bit_exact(out["rgb"][v], ref["rgb"]) and np.array_equal(out["packed"][v], ref["packed"]), (what, v)
            for nme in names:
                a, b = out[nme][v], want[nme]
                assert util.bit_exact(a, b) if a.dtype == np.float32 else np.array_equal(a, b), (what, v, nme)
        assert out["stats"]["primary"] == 2 * ref["stats"]["primary"] and out["stats"]["shadow"] == 2 * ref["stats"]["shadow"], what


def test_graph_replay_reads_the_updated_state(api, monkeypatch):
    """RTX_GRAPH=1: the captured launches carry the block's addresses, the replay reads what the update kernels wrote before it."""
    monkeypatch.setenv("RTX_GRAPH", "1")
    sc, _ = util.load_golden("tori16")
    r = api.Renderer(sc)
    frames = {}
    for f in (2, 3, 2, 3):
        pos, rot = poses("tori16", f)
        p, q = dev(pos), dev(rot)
        for _ in range(3):                      # eager, capture, replay — each after an update of its own
            r.update_instances(p, q)
            out = r.render(serial=True)
        state = r.read_frame_state()
        assert_same_frame(out, oracle_frame(sc, state, f"tori16_f{f}"), f"poses {f}")
        frames.setdefault(f, out)
    assert not np.array_equal(frames[2]["packed"], frames[3]["packed"])


def test_three_contexts_in_flight_on_different_poses(api):
    sc, _ = util.load_golden("tori16")
    rs, keep = [api.Renderer(sc) for _ in range(3)], []
    for rounds in range(3):
        for k, r in enumerate(rs):
            pos, rot = poses("tori16", 1 + k)
            keep.append((dev(pos), dev(rot)))
            r.update_instances(*keep[-1])
            r.render_async(serial=True)
    for k, r in enumerate(rs):
        st, _ = r.stats(); rgb, packed = r.framebuffer()
        state = r.read_frame_state()
        assert_same_frame({"rgb": rgb, "packed": packed, "stats": st}, oracle_frame(sc, state, f"tori16_f{1 + k}"), f"context {k}")


@pytest.mark.parametrize("serial", [False, True])
def test_work_queued_before_the_update_keeps_its_state(api, serial):
    """render, update, render with nothing synchronised in between: view 0 shows the old poses, view 1 the new ones."""
    sc, _ = util.load_golden("tori16")
    old = poses("tori16", 1); new = poses("tori16", 3)
    r = api.Renderer(sc)
    p0, q0, p1, q1 = dev(old[0]), dev(old[1]), dev(new[0]), dev(new[1])
    cams = np.concatenate([sc.camera, sc.camera])
    r.set_views(cams)
    for _ in range(2):                          # the second round updates in place while the first round's frames may still be running
        r.update_instances(p0, q0)
        r.render_views_async(0, 1, serial=serial)
        r.update_instances(p1, q1)
        r.render_views_async(1, 1, serial=serial)
    rgb, packed = r.read_views(0, 2)
    for v, (pos, rot) in enumerate((old, new)):
        ref = oracle_frame(sc, host_state(sc, pos, rot), f"tori16_f{1 if v == 0 else 3}")
        assert util.bit_exact(rgb[v], ref["rgb"]) and np.array_equal(packed[v], ref["packed"]), v
    assert not np.array_equal(packed[0], packed[1])


def test_set_frame_replaces_the_updated_state_and_heatmap_contexts_update(api):
    sc, g = util.load_golden("tori16")
    pos, rot = poses("tori16", 3)
    r = api.Renderer(sc)
    p, q = dev(pos), dev(rot)
    r.update_instances(p, q)
    r.render()
    r.set_frame(sc)
    cmp = util.compare_to_golden(r.render(), g)
    assert cmp["stats_equal"] and cmp["max_abs"] == 0.0 and cmp["packed_mismatch"] == 0, cmp
    sc_h, _ = util.load_golden("tori16"); sc_h.config["heatmap"] = 1
    rh = api.Renderer(sc_h)
    rh.update_instances(p, q)
    out = rh.render()
    ref = api.Renderer(with_state(sc_h, rh.read_frame_state())).render()
    assert_same_frame(out, ref, "heat map")


def test_errors(api):
    sc, _ = util.load_golden("tori16")
    pos, rot = poses("tori16", 1)
    p, q = dev(pos), dev(rot)
    n = len(pos)
    r0 = api.Renderer(sc, upload=False)
    lib = r0.lib
    assert lib.rtx_update_instances(r0.ctx, p.data_ptr(), q.data_ptr(), n) == STATE                # before rtx_set_frame
    assert lib.rtx_read_frame_state(r0.ctx, None, None, None, None) == STATE
    r = api.Renderer(sc)
    assert lib.rtx_update_instances(r.ctx, p.data_ptr(), q.data_ptr(), n - 1) == INVALID           # not the frame's count
    assert lib.rtx_update_instances(r.ctx, p.data_ptr(), q.data_ptr(), 0) == INVALID
    assert lib.rtx_update_instances(r.ctx, None, q.data_ptr(), n) == INVALID
    assert lib.rtx_update_instances(r.ctx, p.data_ptr(), None, n) == INVALID
    assert lib.rtx_update_instances(r.ctx, p.data_ptr() + 2, q.data_ptr(), n) == INVALID           # not 4-byte aligned
    assert lib.rtx_update_instances(r.ctx, p.data_ptr(), q.data_ptr() + 1, n) == INVALID
    assert lib.rtx_update_instances(r.ctx, p.data_ptr(), q.data_ptr(), 65537) == LIMIT
    sc_shallow, _ = util.load_golden("tori16"); sc_shallow.config["stack_size"] = 4               # 16 instances: deepest inner node at depth 3, 5 entries
    r4 = api.Renderer(sc_shallow)
    before = r4.read_frame_state()
    assert lib.rtx_update_instances(r4.ctx, p.data_ptr(), q.data_ptr(), n) == LIMIT                # refused before anything is switched
    assert_state(r4.read_frame_state(), before, "after a refused update")
    with pytest.raises(ValueError):
        r.update_instances(p, q[:-1])
    with pytest.raises(TypeError):
        r.update_instances(p.double(), q)
    with pytest.raises(ValueError):
        r.update_instances(p.cpu(), q.cpu())
    r.update_instances(p, q)                                                                        # the refused calls changed nothing
    assert_state(r.read_frame_state(), host_state(sc, pos, rot))
    r.update_instances(p.data_ptr(), q.data_ptr(), n)                                            # raw device pointers


def hostile_poses():
    """tori16 after two updates with NaN / inf / 1e30 positions and zero, non-unit, NaN and overflowing quaternions for eight instances."""
    pos, rot = poses("tori16", 2)
    pos[1] = (np.nan, 1.0, 2.0); pos[4] = (np.inf, 0.0, 0.0); pos[6] = (1e30, -1e30, 1e30); pos[9] = (-np.inf, np.nan, 3.0)
    rot[2] = (0, 0, 0, 0); rot[3] = (2.0, 0.5, -3.0, 1.5); rot[7] = (np.nan, 0, 0, 1); rot[11] = (1e20, 1e20, 0, 0)
    return pos, rot


def hostile_child():
    """Runs in a process of its own (see test_hostile_poses_keep_the_tree_valid): the hostile poses once through each path."""
    import orc
    from pyrtx import api, host
    sc, _ = util.load_golden("tori16")
    pos, rot = hostile_poses()
    p, q = dev(pos), dev(rot)
    aabbs = np.zeros((len(pos), 6), f32)
    for i in range(len(pos)):
        root = sc.blas[sc.instances["blas_id"][i]].nodes[0]
        _, mn, mx = host.instance_update(pos[i], rot[i], root["aabb_min"], root["aabb_max"], 0)
        aabbs[i, :3] = mn; aabbs[i, 3:] = mx
    want = host_state(sc, pos, rot)
    for small_max in ("1024", "0"):
        os.environ["RTX_UPDATE_SMALL_MAX"] = small_max              # read in rtx_create
        r = api.Renderer(sc)
        r.update_instances(p, q)
        out = r.render()
        inst, nodes, idx = r.read_frame_state()
        # the read-back topology: valid by the CPU test's checks, and the CPU builder's (floats compared with NaN == NaN: the payloads of
        # generated NaNs differ between x86 and gfx950)
        assert check_tree(nodes, idx, aabbs, False) == host.tlas_balanced_inner_depth(len(pos)), small_max
        assert np.array_equal(idx, want[2])
        assert np.array_equal(nodes["left_or_first"], want[1]["left_or_first"]) and np.array_equal(nodes["count"], want[1]["count"])
        for fld in ("aabb_min", "aabb_max"):
            assert util.bit_exact(nodes[fld], want[1][fld]), fld
        for fld in ("world", "world_inv"):
            assert util.bit_exact(inst[fld], want[0][fld]), fld
        ref = orc.OracleScene(with_state(sc, (inst, nodes, idx))).render(threads=8)
        assert_same_frame(out, ref, f"RTX_UPDATE_SMALL_MAX={small_max}")
    print("hostile poses ok")


def test_hostile_poses_keep_the_tree_valid(request):
    """NaN / inf / 1e30 positions and zero, non-unit, NaN and overflowing quaternions for some instances, once through the one-workgroup
    path and once through the multi-launch path: the read-back topology passes the validity checks of the CPU test and equals the CPU
    builder's, and the frame equals the oracle's on that state.  A parity test on legal input.  It runs after the other tests of this
    file and only if none of the session's tests has failed, in a process of its own under its own time limit."""
    assert request.session.testsfailed == 0, "not run: earlier tests of the session failed; find their cause first"
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "hostile-child"], capture_output=True, text=True, timeout=180)
    assert run.returncode == 0 and "hostile poses ok" in run.stdout, (run.returncode, run.stdout[-3000:], run.stderr[-3000:])


if __name__ == "__main__" and sys.argv[1:] == ["hostile-child"]:
    hostile_child()
