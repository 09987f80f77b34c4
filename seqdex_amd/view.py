"""Headless view camera (include/seqdex.h sdx_render_view): camera descriptions, the named cameras, a PNG writer
without dependencies and the frame recorder behind `--record`.  The rendering itself is one HIP kernel (csrc/sdx_camera.hip
k_view_render); this module only describes cameras and moves finished images to disk."""
import json
import os
import struct
import zlib

import numpy as np

from . import _abi

GEOMETRY = {"bounds": _abi.VIEW_BOUNDS, "collision": _abi.VIEW_COLLISION}
CAMERA_NAMES = ("scene", "overview", "wrist")


class ViewCamera:
    """pos / target / up in the env frame, or in the frame of robot link `attach_body` (a row of SDX_T_RB below 24) when it is >= 0;
    hfov_deg: horizontal field of view (pixels are square)"""

    def __init__(self, pos, target, up=(0.0, 0.0, 1.0), attach_body=-1, hfov_deg=90.0):
        self.pos, self.target, self.up = [float(x) for x in pos], [float(x) for x in target], [float(x) for x in up]
        self.attach_body, self.hfov_deg = int(attach_body), float(hfov_deg)
        assert len(self.pos) == 3 and len(self.target) == 3 and len(self.up) == 3

    def to_desc(self, width, height, geometry="collision"):
        d = _abi.ViewDesc()
        d.pos[:], d.target[:], d.up[:] = self.pos, self.target, self.up
        d.attach_body, d.hfov_deg = self.attach_body, self.hfov_deg
        d.width, d.height = int(width), int(height)
        d.geometry = GEOMETRY[geometry] if isinstance(geometry, str) else int(geometry)
        return d

    def basis(self):
        """(f, r, u) of the pinhole model in the camera's own frame (float64; the kernel's is fp32)"""
        f = np.array(self.target) - np.array(self.pos)
        f = f / np.linalg.norm(f)
        r = np.cross(f, np.array(self.up))
        r = r / np.linalg.norm(r)
        return f, r, np.cross(r, f)


def _quat_apply(q, v):
    u, v = np.array(q[:3], float), np.array(v, float)
    t = 2.0 * np.cross(u, v)
    return v + q[3] * t + np.cross(u, t)


def named_camera(name, scene, desc=None):
    """"scene": the Search task's segmentation camera (sdx_scene_desc.seg_cam_*); "overview": a fixed three-quarter view that frames the
    bin, the arm and the base plate; "wrist": on the hand base link at camera_offset_pos, looking along the camera_offset_quat frame's +x
    with its +z up (Isaac Gym's camera convention, GS:887-889)"""
    if isinstance(name, ViewCamera):
        return name
    if name == "scene":
        d = desc if desc is not None else scene.to_desc()
        return ViewCamera(list(d.seg_cam_pos), list(d.seg_cam_target), (0.0, 0.0, 1.0), -1, float(d.seg_cam_hfov_deg))
    if name == "overview":
        return ViewCamera((1.15, -0.80, 1.45), (0.12, -0.02, 0.62), (0.0, 0.0, 1.0), -1, 60.0)
    if name == "wrist":
        p, q = np.array(scene.camera_offset_pos, float), np.array(scene.camera_offset_quat, float)
        q = q / np.linalg.norm(q)
        return ViewCamera(p, p + _quat_apply(q, (1.0, 0.0, 0.0)), _quat_apply(q, (0.0, 0.0, 1.0)), scene.hand_base_body, 90.0)
    raise ValueError("unknown camera %r (one of %s, or a ViewCamera)" % (name, ", ".join(CAMERA_NAMES)))


def parse_size(text):
    """'WxH' -> (W, H)"""
    try:
        w, h = str(text).lower().split("x")
        w, h = int(w), int(h)
    except ValueError:
        raise ValueError("size must look like 256x256, got %r" % (text,))
    if not (1 <= w <= 2048 and 1 <= h <= 2048):
        raise ValueError("size %r outside 1..2048" % (text,))
    return w, h


def _png_chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_bytes(img):
    """8-bit PNG of a uint8 array [H, W] (grey) or [H, W, 3] (RGB): zlib + struct only"""
    a = np.ascontiguousarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError("png_bytes wants uint8 [H, W] or [H, W, 3], got %s %s" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    rows = a.reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()          # filter type 0 in front of every scanline
    ihdr = struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"IDAT", zlib.compress(raw, 6)) + _png_chunk(b"IEND", b"")


def write_png(path, img):
    with open(path, "wb") as f:
        f.write(png_bytes(img))


class Recorder:
    """Frames of chosen envs to disk: capture() renders them (one launch), writes DIR/env%04d/frame%06d.png (and frame%06d_depth.npy with
    save_depth) and appends one line per frame to DIR/frames.jsonl: step, env, frame, progress_buf, reset_buf, reward, file.  `every`: only
    every K-th call captures.  Capturing copies the images to the host, i.e. waits for the device; a run without a recorder never does."""

    def __init__(self, task, directory, envs=(0,), every=1, camera="overview", size=(256, 256), geometry="collision", save_depth=False):
        self.task, self.directory = task, str(directory)
        self.envs = [int(e) for e in envs]
        if not self.envs or min(self.envs) < 0 or max(self.envs) >= task.num_envs:
            raise ValueError("record envs %s outside [0, %d)" % (self.envs, task.num_envs))
        self.every = max(1, int(every))
        self.width, self.height = (parse_size(size) if isinstance(size, str) else (int(size[0]), int(size[1])))
        self.camera = named_camera(camera, task.sim.scene, task.sim._desc)
        self.geometry, self.save_depth = geometry, bool(save_depth)
        self.calls = self.frames = 0
        self._out = None
        self._ids = None
        for e in sorted(set(self.envs)):
            os.makedirs(os.path.join(self.directory, "env%04d" % e), exist_ok=True)
        self._manifest = open(os.path.join(self.directory, "frames.jsonl"), "a")

    def capture(self):
        self.calls += 1
        if (self.calls - 1) % self.every:
            return 0
        import torch
        sim = self.task.sim
        if self._ids is None:
            self._ids = torch.tensor(self.envs, dtype=torch.int32, device=sim.device)
        self._out = sim.render_view(self._ids, self.camera, self.width, self.height, self.geometry, depth=self.save_depth, label=False,
                                    rgb=True, out=self._out)
        rgb = self._out["rgb"].cpu().numpy()
        depth = self._out["depth"].cpu().numpy() if self.save_depth else None
        ids = self._ids.long()
        prog, rst, rew = sim.PROGRESS[ids].cpu().numpy(), sim.RESET[ids].cpu().numpy(), sim.REW[ids].cpu().numpy()
        for k, e in enumerate(self.envs):
            name = os.path.join("env%04d" % e, "frame%06d.png" % self.frames)
            write_png(os.path.join(self.directory, name), rgb[k])
            if depth is not None:
                np.save(os.path.join(self.directory, "env%04d" % e, "frame%06d_depth.npy" % self.frames), depth[k])
            self._manifest.write(json.dumps({"step": self.calls - 1, "env": e, "frame": self.frames, "progress_buf": int(prog[k]),
                                             "reset_buf": int(rst[k]), "reward": float(rew[k]), "file": name}) + "\n")
        self._manifest.flush()
        self.frames += 1
        return len(self.envs)

    def close(self):
        if self._manifest is not None:
            self._manifest.close()
            self._manifest = None
