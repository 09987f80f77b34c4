"""Scene constants of BlockAssemblyGraspSim.

`load_scene()` reads the compact table produced by tools/compile_scene.py from the reference's asset
files (seqdex_amd/scene_data/grasp_sim_scene.json) and exposes it both as python attributes and as
the `sdx_scene_desc` C struct (include/seqdex.h) that sdx_create() takes.  This replaces the scene
construction of the reference's `_create_envs` (GS:523-1058) and `parse_sim_params` (CF:185-217).
"""
import json
import math
import os

import numpy as np

from . import _abi

_DEFAULT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scene_data", "grasp_sim_scene.json")


class Scene:
    def __init__(self, raw):
        self.raw = raw
        rb = raw["robot"]
        bodies = rb["bodies"]
        assert len(bodies) == _abi.NLINK
        self.base_pos, self.base_quat = rb["base_pos"], rb["base_quat"]
        self.parent = [b["parent"] for b in bodies]
        self.link_names = [b["name"] for b in bodies]
        self.lower = np.array([bodies[i + 1]["lower"] for i in range(23)], dtype=np.float32)
        self.upper = np.array([bodies[i + 1]["upper"] for i in range(23)], dtype=np.float32)
        self.hand_base_body = rb["hand_base_body"]
        self.fingertip_bodies = rb["fingertip_bodies"]            # ff, mf, rf, th (GS:183-186)
        self.camera_offset_quat = raw["camera_offset_quat"]
        self.camera_offset_pos = raw["camera_offset_pos"]
        op = raw["vestigial_object_pos"]
        yaw = 1.571                                                # GS:689 from_euler_zyx(0,0,1.571)
        self.object_init_state = [op[0], op[1], op[2], 0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2)] + [0.0] * 6
        # goal_states[:, 0:3] = goal_init_state = object_init_state with z-0.02 (GS:1040-1042), + displacement (GS:1348)
        self.goal_reset_pos = [op[0] - 0.2, op[1] - 0.06, op[2] - 0.02 - 10.12]
        self.brick_types = raw["brick_types"]
        self.statics = raw["statics"]
        self.arm_prepare_pose = [0.0, -0.49826458111314524, -0.01990020486871322, -2.4732269941140346,
                                 -0.01307073642274261, 2.00396583422025, 1.5480939705504309]     # GS:267
        self.finger_reset_unscaled = [0, 0, -1, 0.5, 1, 0, -1, 0.5, 0, 0, -1, 0.5, 0, 0, -1, 0.5]  # GS:1531
        self.insert_pose_a = [-0.1560, -0.2140, -0.2795, -2.1806, -0.0681, 1.9730, 1.1735]       # GS:278
        self.insert_pose_b = [-0.1800, -0.1604, -0.2770, -2.2674, -0.0533, 2.1049, 1.1696]       # GS:281
        # brick type of each of the 132 bricks: 9 layers x 8 types, then the 60 fixed floor bricks
        self.brick_type = [i % 8 for i in range(_abi.NFREE)] + [fb["type"] for fb in raw["fixed_bricks"]]
        self.sim = dict(raw["sim"])
        # solver constants of our own physics definition
        self.solver = dict(friction=1.0, baumgarte=0.2, max_depenetration_vel=1.0, jacobi_relax=1.0, armature=0.0,
                           warm_start=float(os.environ.get("SDX_WARM_START", "0.8")),   # the default since round 3
                           warm_age=float(os.environ.get("SDX_WARM_AGE", "16")))

    # ------------------------------------------------------------------ helpers used by tests / task
    def seg_index(self, env_i):
        """actor index (inside the env) of env i's target brick: brick i%8 with {3,4,7}->0 (GS:962-965)."""
        b = env_i % 8
        return _abi.ACTOR_BRICK0 + (0 if b in (3, 4, 7) else b)

    def spawn_positions(self):
        """the 72 lattice positions of the free bricks, lifted as a whole so that the lowest layer starts 2 mm above the floor slab
        (see to_desc); sets self.spawn_lift"""
        raw = self.raw
        floor = [st for st in self.statics if st["name"] == "brick_floor"]
        lift = 0.0
        if floor:
            top = floor[0]["center"][2] + floor[0]["half"][2]
            low = min(fs["pos"][2] + self.brick_types[fs["type"]]["center"][2] - self.brick_types[fs["type"]]["half"][2] for fs in raw["free_spawn"])
            lift = max(0.0, top + 0.002 - low)
        self.spawn_lift = lift
        return [[fs["pos"][0], fs["pos"][1], fs["pos"][2] + lift] for fs in raw["free_spawn"]]

    def to_desc(self, **overrides):
        d = _abi.SceneDesc()
        raw, rb = self.raw, self.raw["robot"]
        d.abi_version = _abi.SDX_ABI_VERSION
        d.base_pos[:] = self.base_pos
        d.base_quat[:] = self.base_quat
        for i, b in enumerate(rb["bodies"]):
            d.parent[i] = b["parent"]
            d.joint_pos[i][:] = b.get("joint_pos", [0, 0, 0])
            d.joint_quat[i][:] = b.get("joint_quat", [0, 0, 0, 1])
            d.joint_axis[i][:] = b.get("axis", [0, 0, 1])
            d.link_mass[i] = b["mass"]
            d.link_com[i][:] = b["com"]
            I = b["inertia"]
            d.link_inertia[i][:] = [I[0][0], I[1][1], I[2][2], I[0][1], I[0][2], I[1][2]]
        for j in range(23):
            dj = rb["dof"][j]
            d.lower[j], d.upper[j] = float(self.lower[j]), float(self.upper[j])
            d.kp[j], d.kd[j], d.effort[j], d.vel_limit[j] = dj["kp"], dj["kd"], dj["effort"], dj["vel_limit"]
            d.armature[j] = self.solver["armature"]
        k = 0
        for i, b in enumerate(rb["bodies"]):
            for bx in b["boxes"]:
                assert k < _abi.MAX_RBOX
                d.rbox_link[k] = i
                d.rbox_center[k][:] = bx["center"]
                d.rbox_quat[k][:] = bx["quat"]
                d.rbox_half[k][:] = bx["half"]
                k += 1
        d.n_rbox = k
        for t, bt in enumerate(self.brick_types):
            d.brick_half[t][:] = bt["half"]
            d.brick_center[t][:] = bt["center"]
            d.brick_com[t][:] = bt["com"]
            d.brick_mass[t] = bt["mass"]
            d.brick_inertia[t][:] = bt["inertia_diag"]
            assert len(bt["sub"]) <= _abi.MAX_SUB and len(bt["hollow"]) <= _abi.MAX_SUB_HOLLOW
            d.brick_nsub[t] = len(bt["sub"])
            for k, bx in enumerate(bt["sub"]):
                d.brick_sub_center[t][k][:] = bx["center"]
                d.brick_sub_half[t][k][:] = bx["half"]
            d.hollow_nsub[t] = len(bt["hollow"])
            for k, bx in enumerate(bt["hollow"]):
                d.hollow_sub_center[t][k][:] = bx["center"]
                d.hollow_sub_half[t][k][:] = bx["half"]
        d.seg_hollow = 0
        d.brick_type[:] = self.brick_type
        d.n_static = len(self.statics)
        assert d.n_static <= _abi.MAX_STATIC
        nsub = 0
        for s, st in enumerate(self.statics):
            d.static_center[s][:] = st["center"]
            d.static_half[s][:] = st["half"]
            boxes = [(st["center"], st["half"])]
            if st["name"] == "base_plate":           # body + studs (tools/compile_scene.py::plate_compound), GS:810-838
                pp = raw["base_plate_pos"]
                boxes = [([pp[i] + bx["center"][i] for i in range(3)], bx["half"]) for bx in raw["base_plate"]["sub"]]
            nsub = self._add_static_subs(d, s, boxes, nsub)
        d.n_static_sub = nsub
        d.object_init_state[:] = self.object_init_state
        d.goal_reset_pos[:] = self.goal_reset_pos
        for s in range(6):                      # table + 5 bin walls are the first six statics
            d.static_actor_pos[s][:] = self.statics[s]["center"]
        d.base_plate_pos[:] = raw["base_plate_pos"]
        for i, fb in enumerate(raw["fixed_bricks"]):
            d.fixed_brick_pos[i][:] = fb["pos"]
        # The reference spawns the lowest layer of free bricks at z = 0.62 (GS:737-742), INSIDE its floor of fixed bricks (z = 0.625,
        # GS:766-777), and lets PhysX push them out; a brick that overlaps the floor slab by its whole height has no meeting face in
        # this engine (top samples just above the slab, bottom samples pushed down) and stays there - round 3
        # found every target brick of the synthetic piles buried that way.  The lattice is lifted so that its lowest layer starts
        # 2 mm above the floor; the piles then settle ON it, as the reference's saved pile states do.
        for i, pos in enumerate(self.spawn_positions()):
            d.free_spawn_pos[i][:] = pos
        d.free_spawn_quat[:] = raw["free_spawn"][0]["quat"]
        d.hand_base_body = self.hand_base_body
        d.fingertip_body[:] = self.fingertip_bodies
        d.camera_offset_quat[:] = self.camera_offset_quat
        d.camera_offset_pos[:] = self.camera_offset_pos
        d.arm_prepare_pose[:] = self.arm_prepare_pose
        d.finger_reset_unscaled[:] = self.finger_reset_unscaled
        d.insert_pose_a[:] = self.insert_pose_a
        d.insert_pose_b[:] = self.insert_pose_b
        d.max_episode_length, d.act_moving_average, d.av_factor = 150.0, 1.0, 0.1
        d.clip_obs, d.clip_actions = 5.0, 1.0
        d.dt, d.substeps, d.solver_iters = self.sim["dt"], self.sim["substeps"], self.sim["pos_iters"]
        d.contact_offset = self.sim["contact_offset"]
        d.gravity[:] = self.sim["gravity"]
        d.friction, d.baumgarte = self.solver["friction"], self.solver["baumgarte"]
        d.max_depenetration_vel, d.jacobi_relax = self.solver["max_depenetration_vel"], self.solver["jacobi_relax"]
        d.warm_start, d.warm_age = self.solver["warm_start"], self.solver["warm_age"]
        d.orient_tvalue_gate = 0.99                        # OR:1203
        d.robot_angular_damping = 0.01                     # GS:546 (asset_options.angular_damping of the arm-hand asset)
        d.grasp_tvalue_gate = 0.8                          # GS:1406
        d.task_kind = _abi.TASK_GRASP                     # the tasks of seqdex_amd/tasks/ override it with their TASK_KIND
        d.target_euler[:] = [0.0, 3.1415, 1.571]          # OR:477
        d.seg_mass_scale = 1.0                            # GS:980-981 (x1); Orient x50 (OR:977)
        d.static_var_slot = -1
        d.static_var_row[:] = [0, 0, 0]
        d.seg_cam_pos[:] = [0.35, 0.19, 1.0]              # gym.set_camera_location(camera, env, Vec3(0.35, 0.19, 1.0), Vec3(0.2, 0.19, 0)), SE:875
        d.seg_cam_target[:] = [0.2, 0.19, 0.0]
        d.seg_cam_hfov_deg = 90.0                         # gymapi.CameraProperties default horizontal_fov
        d.search_default_arm[:] = [0.9467, -0.5708, -2.4997, -2.3102, -0.7739, 2.6616, 0.6497]     # SE:203
        d.search_finger_pose[:] = [0.0, -0.174, 0.785, 0.785] * 4                                 # SE:205-206,220-222
        for k_, v in overrides.items():
            if hasattr(v, "__len__") and not isinstance(v, (str, bytes)):
                getattr(d, k_)[:] = list(v)
            else:
                setattr(d, k_, v)
        if d.task_kind == _abi.TASK_INSERT:
            self._place_insert_plates(d, overrides.get("seg_hollow", 1))
        return d

    @staticmethod
    def _add_static_subs(d, row, boxes, nsub):
        assert nsub + len(boxes) <= _abi.MAX_STATIC_SUB
        d.static_sub_first[row], d.static_sub_n[row] = nsub, len(boxes)
        for c, h in boxes:
            d.static_sub_center[nsub][:] = c
            d.static_sub_half[nsub][:] = h
            nsub += 1
        return nsub

    INSERT_PLATE_MARGIN = 0.004

    def _place_insert_plates(self, d, seg_hollow=1):
        """BlockAssemblyInsertSim: the base plate actor sits at (0.25, -0.2, 0.618) (IS:1438-1440; the torch_rand_int(0, 1) offsets
        are always 0) and is one of 4x4x{1,2,4} by env % 3 (IS:971-977): three rows of the static-body table, each a stud compound
        (tools/compile_scene.py::plate_compound), shown in the base plate's slot by env % 3.  The plate and its 4 x 4 studs are
        symmetric under the 0 / 90 degree yaw drawn at each reset (IS:1435-1436).  The hollow compound of the target brick (walls,
        roof) takes the studs: seg_hollow = 1 (the reference runs V-HACD on the bricks of this task, IS:698-709)."""
        raw = self.raw
        ps = [i for i, st in enumerate(self.statics) if st["name"] == "base_plate"][0]
        pos = raw["insert_plate_pos"]
        d.base_plate_pos[:] = pos
        # bricks that end flush with the plate edge (the 1x4 brick spans it; the 1x3 brick of the env % 8 == 5 rule ends on it) would
        # touch the plate's SIDE faces with their corner samples and get no vertical support from the sampled box contacts
        # (DESIGN.md section 3); the body box is widened by 4 mm per side so that those corners land on the top face
        m = self.INSERT_PLATE_MARGIN
        nsub = d.static_sub_first[ps]                       # the plate is the last static: its boxes are replaced, the variants follow
        assert ps == d.n_static - 1
        d.static_var_slot = ps
        for k, pl in enumerate(raw["insert_plates"]):
            row = ps if k == 0 else d.n_static + k - 1
            assert row < _abi.MAX_STATIC_TAB
            d.static_center[row][:] = [pos[i] + pl["center"][i] for i in range(3)]
            d.static_half[row][:] = [pl["half"][0] + m, pl["half"][1] + m, pl["half"][2]]
            boxes = [([pos[i] + bx["center"][i] for i in range(3)], list(bx["half"])) for bx in pl["sub"]]
            boxes[0] = (boxes[0][0], [boxes[0][1][0] + m, boxes[0][1][1] + m, boxes[0][1][2]])
            nsub = self._add_static_subs(d, row, boxes, nsub)
            d.static_var_row[k] = row
        d.n_static_sub = nsub
        d.seg_hollow = seg_hollow


def load_scene(path=None):
    with open(path or _DEFAULT) as f:
        return Scene(json.load(f))
