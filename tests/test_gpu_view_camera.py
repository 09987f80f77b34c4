"""-m gpu: the view camera (include/seqdex.h sdx_render_view) on the HIP path against its numpy restatement
(tests/helpers/view_oracle.py) under the share rule, against the Search task's own segmentation image, and its promise not to disturb a
run; `--record` end to end.  PARITY UNPINNED against Isaac Gym's renderer (closed source), as for the segmentation camera."""
import json
import os
import struct
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import camera_oracle as CO  # noqa: E402
from seqdex_amd import view as V  # noqa: E402
from tests.helpers import view_oracle as VO  # noqa: E402

SHARE = 0.003      # silhouette flips of this ray caster
N = 8


def _sim(kind, **kw):
    """8 envs, the free bricks scattered over the bin, the hand over it"""
    from seqdex_amd.sim import SdxSim
    s = SdxSim(N, device="cuda:0", seed=22 if kind == 2 else 2, task_kind=kind, **kw)
    s.ROOT.view(N, 142, 13)[:, 9:81, :7] = torch.as_tensor(VO.scattered_bricks(N)).cuda()
    arm = torch.tensor(s.scene.arm_prepare_pose[:7], dtype=torch.float32)
    if kind == 3:
        arm[1] += 0.35      # shoulder lowered: the hand comes down into the frustum of Search's camera, which looks down from z = 1 m
    s.DOF.view(N, 23, 2)[:, :7, 0] = arm.cuda()
    s.refresh_kinematics()
    torch.cuda.synchronize()
    return s


@pytest.fixture(scope="module")
def grasp8():
    s = _sim(0)
    yield s
    s.close()


def _check(s, ids, camera, W, H, geometry, out):
    root, rb = s.ROOT.view(N, 142, 13).cpu().numpy(), s.RB.cpu().numpy()
    cam = V.named_camera(camera, s.scene, s._desc)
    got_all = {k: v.cpu().numpy() for k, v in out.items() if k != "_ids"}
    wants = []
    for k, e in enumerate(ids):
        want = VO.render(s._desc, root[e], rb[e], e, cam, W, H, VO.COLLISION if geometry == "collision" else VO.BOUNDS)
        got = tuple(got_all[key][k] if key in got_all else None for key in ("depth", "label", "rgb"))
        share = VO.failing_share(got, want)
        labels = np.unique(got[1])
        print("env %d camera %s %dx%d %s: failing share %.5f, %d labels" % (e, camera, W, H, geometry, share, len(labels)))
        assert share <= SHARE, (e, share)
        assert len(labels) > 20 and ((labels < 0) & (labels > -100)).any(), labels          # an empty image cannot pass
        wants.append(want)
    return got_all, wants


def test_bounds_scene_camera_is_the_segmentation_camera(scene):
    s = _sim(3)
    try:
        s.ROOT.view(N, 142, 13)[3, scene.seg_index(3), 0:3] = torch.tensor([3.0, 3.0, 0.3]).cuda()
        s.refresh_kinematics()
        s.render_segmentation()
        ids = [0, 3, 5]
        out = s.render_view(ids, "scene", 128, 128, "bounds")
        torch.cuda.synchronize()
        got, wants = _check(s, ids, "scene", 128, 128, "bounds", out)
        seg = s.SEG_IMAGE.cpu().numpy()
        root, rb = s.ROOT.view(N, 142, 13).cpu().numpy(), s.RB.cpu().numpy()
        for k, e in enumerate(ids):
            mine = np.maximum(got["label"][k], 0)
            a, b = float((mine != seg[e]).mean()), float((mine != CO.render(s._desc, root[e], rb[e])).mean())
            print("env %d: differs from SDX_T_SEG_IMAGE on %.5f, from camera_oracle on %.5f of the pixels" % (e, a, b))
            assert a <= SHARE and b <= SHARE, (e, a, b)
    finally:
        s.close()


def test_overview_collision_subset_odd_size(grasp8):
    out = grasp8.render_view([5, 0, 3], "overview", 100, 52, "collision")
    torch.cuda.synchronize()
    _check(grasp8, [5, 0, 3], "overview", 100, 52, "collision", out)


def test_wrist_camera(grasp8):
    out = grasp8.render_view(list(range(N)), "wrist", 80, 80, "collision")
    torch.cuda.synchronize()
    _check(grasp8, [0, 6], "wrist", 80, 80, "collision", {k: v[[0, 6]] for k, v in out.items() if k != "_ids"})


def test_insert_sim_three_plates():
    s = _sim(2, max_episode_length=125.0)
    try:
        out = s.render_view([0, 1, 2], "overview", 96, 64, "collision")
        torch.cuda.synchronize()
        got, wants = _check(s, [0, 1, 2], "overview", 96, 64, "collision", out)
        plate = (wants[0][1] == -107) | (wants[1][1] == -107) | (wants[2][1] == -107)
        d = got["depth"]
        assert plate.any() and (d[0][plate] != d[1][plate]).any() and (d[1][plate] != d[2][plate]).any()
    finally:
        s.close()


def test_rendering_leaves_the_state_alone(grasp8):
    s = grasp8
    before = {k: s.tensor(k).clone() for k in ("ROOT", "RB", "DOF", "OBS")}
    for cam, geo in (("overview", "collision"), ("wrist", "bounds")):
        s.render_view([1, 7, 1], cam, 72, 40, geo)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(s.tensor(k), v), k


def test_recorder_on_or_off_same_run(tmp_path):
    import yaml
    from seqdex_amd.tasks.block_assembly_grasp_sim import BlockAssemblyGraspSim
    from seqdex_amd.vec_task_rlgames import RLgamesVecTaskPython
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = torch.Generator().manual_seed(0)
    actions = [((torch.rand(16, 23, generator=g) * 2 - 1) * 0.5).cuda() for _ in range(8)]
    runs = []
    for record in (False, True):
        cfg = yaml.safe_load(open(os.path.join(root_dir, "seqdex_amd/cfg/allegro_hand_block_assembly_grasp_sim.yaml")))
        cfg["env"]["numEnvs"] = 16
        task = BlockAssemblyGraspSim(cfg, device_type="cuda", device_id=0, headless=True, seed=5, piles_per_type=2)
        env = RLgamesVecTaskPython(task, "cuda:0")
        if record:
            env.recorder = V.Recorder(task, tmp_path, envs=[0, 9], every=2, camera="wrist", size=(48, 32), save_depth=True)
        trace = []
        for a in actions:
            env.step(a)
            trace.append([task.sim.OBS.clone(), task.sim.REW.clone(), task.sim.RESET.clone()])
        torch.cuda.synchronize()
        runs.append(trace)
        if record:
            assert env.recorder.frames == 4 and len(open(tmp_path / "frames.jsonl").read().splitlines()) == 8
            assert np.load(tmp_path / "env0009" / "frame000003_depth.npy").shape == (32, 48)
            env.recorder.close()
        task.sim.close()
    for t, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), t


def _png_size_and_pixels(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    w, h = struct.unpack(">II", data[16:24])
    n = struct.unpack(">I", data[33:37])[0]
    assert data[37:41] == b"IDAT"
    raw = np.frombuffer(zlib.decompress(data[41:41 + n]), np.uint8).reshape(h, 1 + 3 * w)
    return w, h, raw[:, 1:]


def test_train_rlgames_record_play(tmp_path):
    from seqdex_amd.config import get_args
    from seqdex_amd.train_rlgames import build
    rec = tmp_path / "rec"
    args = get_args(["--task=BlockAssemblyGraspSim", "--num_envs=16", "--play", "--headless", "--episode_length", "4", "--record", str(rec),
                     "--record_envs", "0,3", "--logdir", str(tmp_path)])
    t, env, agent, logdir, rank = build(args, task_kwargs={"piles_per_type": 2}, minibatch_size=64)
    agent.play(games_num=1)
    torch.cuda.synchronize()
    lines = [json.loads(x) for x in open(rec / "frames.jsonl").read().splitlines()]
    frames = env.recorder.frames
    assert frames >= 4 and len(lines) == 2 * frames and {x["env"] for x in lines} == {0, 3}
    for x in lines:
        assert {"step", "env", "progress_buf", "reset_buf", "reward", "file"} <= set(x)
        w, h, pix = _png_size_and_pixels(rec / x["file"])
        assert (w, h) == (256, 256) and pix.min() != pix.max()
    assert sorted(os.listdir(rec / "env0003")) == ["frame%06d.png" % i for i in range(frames)]
    assert t.render() is None
    img = t.render(mode="rgb_array", env=3, camera="overview", width=64, height=48)
    assert img.shape == (48, 64, 3) and img.dtype == np.uint8 and img.min() != img.max()
    assert t.render(mode="depth_array", width=32, height=16).dtype == np.float32 and t.render(mode="label_array", width=32, height=16).dtype == np.int16
    agent.ppo.close() if hasattr(agent.ppo, "close") else None
    t.sim.close()
