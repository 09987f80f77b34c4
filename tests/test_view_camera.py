"""CPU: the view camera (include/seqdex.h sdx_render_view).  Known answers of its numpy restatement
(tests/helpers/view_oracle.py) and its pin to oracle/camera_oracle.py; the kernel SOURCE (csrc/sdx_camera.hip k_view_render) on the SIMT
emulator against that restatement under the share rule; the host side (PNG writer, named cameras, flags, render())."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import camera_oracle as CO  # noqa: E402
from seqdex_amd import _abi  # noqa: E402
from seqdex_amd import view as V  # noqa: E402
from tests.helpers import view_oracle as VO  # noqa: E402

SHARE = 0.003      # silhouette flips of this ray caster


# ------------------------------------------------------------------ 1. the helper
def _one_box(extra=None, W=33, H=33, hfov=90.0):
    c, q, h = [[2.0, 0.0, 0.0]], [[0, 0, 0, 1]], [[0.5, 0.4, 0.4]]
    lab, cls = [7], [VO.C_TYPE0 + 3]
    if extra is not None:
        c.append(extra[0]); q.append([0, 0, 0, 1]); h.append(extra[1]); lab.append(9); cls.append(VO.C_FIXED)
    cam = V.ViewCamera((0, 0, 0), (1, 0, 0), (0, 0, 1), -1, hfov)
    origin, f, r, u = VO.camera_basis(cam, None)
    return VO.render_boxes(np.array(c, np.float32), np.array(q, np.float32), np.array(h, np.float32), np.array(lab), np.array(cls),
                           origin, f, r, u, hfov, W, H)


def test_helper_box_straight_ahead():
    depth, label, rgb, axis = _one_box()
    assert depth[16, 16] == np.float32(1.5) and label[16, 16] == 7 and axis[16, 16] == 0       # the face x = 1.5, entered along the box's x axis
    np.testing.assert_array_equal(rgb[16, 16], VO.COLORS[VO.C_TYPE0 + 3].astype(np.uint8))      # head on: class colour x 1.0
    assert np.isinf(depth[0, 0]) and label[0, 0] == 0
    np.testing.assert_array_equal(rgb[0, 0], VO.COLORS[0].astype(np.uint8))                     # background, unshaded
    on = label == 7
    assert (depth[on] == np.float32(1.5)).all()                                                 # depth = distance along the optical axis, not along the ray
    assert rgb[on].min() < rgb[16, 16].min()                                                    # off-axis pixels are shaded


def test_helper_camera_inside_a_box_sees_through_it():
    plain = _one_box()
    boxed = _one_box(extra=([0.1, 0.0, 0.0], [1.0, 1.0, 1.0]))                                  # strictly contains the ray origin
    for a, b in zip(plain, boxed):
        np.testing.assert_array_equal(a, b)
    hit = _one_box(extra=([1.0, 0.0, 0.0], [0.2, 1.0, 1.0]))                                    # the same box in front of the camera is drawn
    assert hit[1][16, 16] == 9 and hit[0][16, 16] == np.float32(0.8)


def test_helper_non_square_image_has_square_pixels():
    depth, label, rgb, axis = _one_box(W=64, H=32)
    on = label == 7
    wide, high = on[16].sum(), on[:, 32].sum()          # the 0.8 m x 0.8 m face at 1.5 m: as many columns as rows
    assert wide == high and 16 <= wide <= 18, (wide, high)      # 0.8 / 1.5 / (2 / 64) = 17.07 pixels


@pytest.fixture(scope="module")
def emu():
    from tests.hipemu.sim import EmuSim
    sims = {}

    def get(kind, **kw):
        if kind not in sims:
            s = EmuSim(3, seed=22, task_kind=kind, **kw)
            vp = C.c_void_p
            s.lib.sdx_render_view.argtypes = [vp, C.POINTER(_abi.ViewDesc), vp, C.c_int32, vp, vp, vp, vp]
            s.lib.sdx_render_view.restype = C.c_int32
            s.ROOT.view(3, 142, 13)[:, 9:81, :7] = torch.as_tensor(VO.scattered_bricks(3))
            s.DOF.view(3, 23, 2)[:, :7, 0] = torch.tensor(s.scene.arm_prepare_pose[:7], dtype=torch.float32)     # the hand over the bin
            s.refresh_kinematics()
            sims[kind] = s
        return sims[kind]
    yield get
    for s in sims.values():
        s.close()


def test_helper_bounds_scene_camera_equals_camera_oracle(emu):
    s = emu(3)
    root, rb = s.ROOT.view(3, 142, 13).numpy(), s.RB.numpy()
    cam = V.named_camera("scene", s.scene, s._desc)
    for e in (0, 2):
        depth, label, rgb, axis = VO.render(s._desc, root[e], rb[e], e, cam, 128, 128, VO.BOUNDS)
        want = CO.render(s._desc, root[e], rb[e])
        np.testing.assert_array_equal(np.maximum(label, 0), want)
        assert len(np.unique(want)) > 20


# ------------------------------------------------------------------ 2. the kernel source on the emulator
W, H = 40, 24      # 3 x 2 tiles of 16 x 16: edge tiles in both directions


def _check(s, ids, camera, out, geometry=VO.COLLISION):
    root, rb = s.ROOT.view(3, 142, 13).numpy(), s.RB.numpy()
    cam = V.named_camera(camera, s.scene, s._desc)
    wants = []
    for k, e in enumerate(ids):
        want = VO.render(s._desc, root[e], rb[e], e, cam, W, H, geometry)
        got = tuple(out[key][k].numpy() if key in out else None for key in ("depth", "label", "rgb"))
        share = VO.failing_share(got, want)
        print("env %d camera %s: failing share %.5f, %d labels" % (e, camera, share, len(np.unique(want[1]))))
        assert share <= SHARE, (e, share)
        wants.append(want)
    return wants


def test_emulated_kernel_overview_collision(emu):
    s = emu(0)
    wants = _check(s, [0, 1, 2], "overview", s.render_view([0, 1, 2], "overview", W, H, "collision"))
    for w in wants:
        assert len(np.unique(w[1])) > 20 and ((w[1] < 0) & (w[1] > -100)).any()


def test_emulated_kernel_insert_sim_three_plates(emu):
    s = emu(2, max_episode_length=125.0)
    assert s._desc.static_var_slot == 7 and s._desc.seg_hollow == 1
    out = s.render_view([0, 1, 2], "overview", W, H, "collision")
    wants = _check(s, [0, 1, 2], "overview", out)
    plate = [(w[1] == -107) for w in wants]
    assert all(p.any() for p in plate)
    d = out["depth"].numpy()
    region = plate[0] | plate[1] | plate[2]
    assert (d[0][region] != d[1][region]).any() and (d[1][region] != d[2][region]).any()      # 4x4x1, 4x4x2, 4x4x4 by env % 3


def test_emulated_kernel_wrist_camera(emu):
    s = emu(0)
    wants = _check(s, [0, 1, 2], "wrist", s.render_view([0, 1, 2], "wrist", W, H, "collision"))
    for w in wants:
        assert len(np.unique(w[1])) > 20 and (w[1] > 0).any() and (w[1] <= -100).any()              # the bricks and the bin below the hand


def test_emulated_kernel_env_subset_with_repeats(emu):
    s = emu(0)
    out = s.render_view([2, 0, 2], "overview", W, H, "collision")
    _check(s, [2, 0, 2], "overview", out)
    np.testing.assert_array_equal(out["label"][0].numpy(), out["label"][2].numpy())
    assert (out["label"][0].numpy() != out["label"][1].numpy()).any()


def test_emulated_kernel_depth_only_and_bounds(emu):
    s = emu(0)
    out = s.render_view([0, 1, 2], "overview", W, H, "collision", label=False, rgb=False)
    assert set(out) - {"_ids"} == {"depth"}
    _check(s, [0, 1, 2], "overview", out)
    _check(s, [1], "scene", s.render_view([1], "scene", W, H, "bounds"), VO.BOUNDS)


def test_render_view_argument_errors(emu):
    s = emu(0)
    ids = torch.zeros(1, dtype=torch.int32)
    buf = torch.zeros(64 * 64, dtype=torch.float32)

    def call(n=1, **kw):
        cam = V.ViewCamera(kw.pop("pos", (1, 0, 1)), kw.pop("target", (0, 0, 0)), kw.pop("up", (0, 0, 1)), kw.pop("attach_body", -1))
        d = cam.to_desc(kw.pop("width", 16), kw.pop("height", 16), kw.pop("geometry", "collision"))
        rc = s.lib.sdx_render_view(s.h, C.byref(d), C.c_void_p(ids.data_ptr()), n, C.c_void_p(buf.data_ptr()), None, None, None)
        return rc, s.lib.sdx_last_error(s.h).decode()

    assert call()[0] == 0
    for kw in (dict(width=0), dict(height=2049), dict(attach_body=24), dict(attach_body=-2), dict(target=(1, 0, 1)), dict(up=(2, 0, 2)),
               dict(up=(0, 0, 0)), dict(geometry=2), dict(n=-1)):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("sdx_render_view:"), (kw, rc, msg)
    assert call(n=0)[0] == 0


# ------------------------------------------------------------------ 3. host logic
def _decode_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, inter = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, inter) == (8, 0, 0, 0) and ctype in (0, 2)
    ch = 3 if ctype == 2 else 1
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * ch)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape((h, w, 3) if ch == 3 else (h, w))


def test_png_writer_round_trips(tmp_path):
    rng = np.random.default_rng(0)
    for shape in ((5, 7, 3), (52, 100, 3), (9, 4)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        np.testing.assert_array_equal(_decode_png(V.png_bytes(img)), img)
    V.write_png(str(tmp_path / "a.png"), np.zeros((3, 2, 3), np.uint8))
    assert _decode_png((tmp_path / "a.png").read_bytes()).shape == (3, 2, 3)
    with pytest.raises(ValueError):
        V.png_bytes(np.zeros((3, 3), np.float32))


def test_named_cameras_have_orthonormal_bases(scene):
    for name in V.CAMERA_NAMES:
        cam = V.named_camera(name, scene)
        f, r, u = cam.basis()
        m = np.stack([f, r, u])
        assert np.isfinite(m).all()
        np.testing.assert_allclose(m @ m.T, np.eye(3), atol=1e-9)
        assert 0 < cam.hfov_deg < 180
    assert V.named_camera("wrist", scene).attach_body == scene.hand_base_body and V.named_camera("overview", scene).attach_body == -1
    d = scene.to_desc()
    assert V.named_camera("scene", scene, d).pos == [float(x) for x in d.seg_cam_pos]
    with pytest.raises(ValueError):
        V.named_camera("nowhere", scene)


def test_record_flags_parse():
    from seqdex_amd.config import get_args
    a = get_args([])
    assert a.record == "" and a.record_envs == [0] and a.record_every == 1 and a.record_camera == "overview" and a.record_size == (256, 256)
    a = get_args(["--record", "out", "--record_envs", "0,3", "--record_every", "5", "--record_camera", "wrist", "--record_size", "100x52"])
    assert (a.record, a.record_envs, a.record_every, a.record_camera, a.record_size) == ("out", [0, 3], 5, "wrist", (100, 52))
    for bad in (["--record_size", "100"], ["--record_envs", "a"], ["--record_camera", "top"], ["--record_every", "0"], ["--record_size", "0x4"]):
        with pytest.raises(SystemExit):
            get_args(bad)


def test_render_without_mode_is_none():
    from seqdex_amd.tasks.block_assembly_grasp_sim import BlockAssemblyGraspSim
    from seqdex_amd.tasks.block_assembly_insert_sim import BlockAssemblyInsertSim
    from seqdex_amd.tasks.block_assembly_orient import BlockAssemblyOrient
    from seqdex_amd.tasks.block_assembly_search import BlockAssemblySearch
    for cls in (BlockAssemblyGraspSim, BlockAssemblyInsertSim, BlockAssemblyOrient, BlockAssemblySearch):
        assert cls.render is BlockAssemblyGraspSim.render
        assert cls.render(object()) is None and cls.render(object(), True) is None
