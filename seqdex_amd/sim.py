"""Thin Python binding of the sdx_* C ABI (include/seqdex.h): owns a handle and exposes the library-owned
device buffers as zero-copy torch tensors — the equivalent of `gymtorch.wrap_tensor(gym.acquire_*_tensor(sim))`
(GS:237-241,313-322).  torch is plumbing here (device pointers, streams); all arithmetic is in libseqdex_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi
from .scene import load_scene

_TORCH_DTYPE = {0: (torch.float32, "<f4"), 1: (torch.int64, "<i8"), 2: (torch.int32, "<i4"), 3: (torch.uint8, "|u1"),
                4: (torch.float64, "<f8"), 5: (torch.int16, "<i2")}


class _DevArray:
    """minimal __cuda_array_interface__ carrier so torch can alias a raw device pointer (ROCm uses the same protocol)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


def wrap_device_pointer(ptr, shape, dtype_code, device):
    tdt, typestr = _TORCH_DTYPE[dtype_code]
    t = torch.as_tensor(_DevArray(ptr, shape, typestr), device=device)
    assert t.data_ptr() == ptr and t.dtype == tdt
    return t


def _stream_ptr(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class SdxError(RuntimeError):
    pass


class SimState:
    """Device memory for `rows` env states of one simulator layout (include/seqdex.h sdx_state_*): made by SdxSim.snapshot().  save() /
    restore() are stream-ordered single launches; a run continues from a restored state bit for bit.  Not in a snapshot: the logs (rings,
    CONTACT_STATS, DEBUG), the launch-order hints and configuration (piles, T-value weights, the randomization descriptor)."""

    def __init__(self, sim, rows):
        self.sim, self.rows = sim, int(rows)
        s = C.c_void_p()
        sim._check(sim.lib.sdx_state_create(sim.h, C.c_int32(self.rows), C.byref(s)))
        self.s = s
        self._row_env = {}        # row -> source env of the saves made with host lists (None: saved through a device tensor)
        self._keep = None

    def save(self, env_ids=None, rows=None, sim=None):
        """env env_ids[i] -> row rows[i] (rows None: row i); env_ids None: every env plus the global state (save_all)"""
        sim = sim or self.sim
        if env_ids is None:
            if rows is not None:
                raise ValueError("SimState.save: rows without env_ids")
            sim._check(sim.lib.sdx_state_save_all(sim.h, self.s, sim._stream_or_none()))
            self._row_env = {e: e for e in range(sim.num_envs)}
            return
        e, he = sim._ids(env_ids, "SimState.save: env_ids", sim.num_envs)
        n = int(e.numel())
        if rows is None:
            if n > self.rows:
                raise ValueError("SimState.save: %d envs into %d rows" % (n, self.rows))
            r, hr, rp = None, list(range(n)), None
        else:
            r, hr = sim._ids(rows, "SimState.save: rows", self.rows, unique=True)
            rp = C.c_void_p(r.data_ptr())
            if int(r.numel()) != n:
                raise ValueError("SimState.save: %d envs for %d rows" % (n, int(r.numel())))
        sim._check(sim.lib.sdx_state_save(sim.h, self.s, C.c_void_p(e.data_ptr()), rp, C.c_int32(n), sim._stream_or_none()))
        if hr is not None:
            for i, row in enumerate(hr):
                self._row_env[row] = he[i] if he is not None else None
        else:
            self._row_env = {row: None for row in range(self.rows)}
        self._keep = (e, r)

    def restore(self, rows=None, env_ids=None, sim=None):
        """row rows[i] -> env env_ids[i] (rows None: row i); both None: every env plus the global state (restore_all).  `sim`: another
        simulator of the same layout (default: the one the snapshot was made by)"""
        sim = sim or self.sim
        if env_ids is None:
            if rows is not None:
                raise ValueError("SimState.restore: rows without env_ids")
            sim._check(sim.lib.sdx_state_restore_all(sim.h, self.s, sim._stream_or_none()))
            return
        e, he = sim._ids(env_ids, "SimState.restore: env_ids", sim.num_envs, unique=True)
        n = int(e.numel())
        if rows is None:
            if n > self.rows:
                raise ValueError("SimState.restore: %d envs from %d rows" % (n, self.rows))
            r, hr, rp = None, list(range(n)), None
        else:
            r, hr = sim._ids(rows, "SimState.restore: rows", self.rows)
            rp = C.c_void_p(r.data_ptr())
            if int(r.numel()) != n:
                raise ValueError("SimState.restore: %d rows for %d envs" % (int(r.numel()), n))
        if hr is not None and he is not None:
            for row, env in zip(hr, he):
                if row not in self._row_env:
                    raise ValueError("SimState.restore: row %d was never saved" % row)
                src = self._row_env[row]
                if src is not None and sim.env_class(src) != sim.env_class(env):
                    raise ValueError("SimState.restore: row %d holds env %d, which is not of env %d's class" % (row, src, env))
        sim._check(sim.lib.sdx_state_restore(sim.h, self.s, rp, C.c_void_p(e.data_ptr()), C.c_int32(n), sim._stream_or_none()))
        self._keep = (e, r)

    def close(self):
        if getattr(self, "s", None) is not None and self.s.value:
            self.sim.lib.sdx_state_destroy(self.s)
            self.s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SdxSim:
    """One simulator+task instance on one GPU (one process per GPU; envs shard across ranks)."""

    def __init__(self, num_envs, device="cuda:0", seed=22, scene=None, desc=None, **desc_overrides):
        """desc: a ready sdx_scene_desc (Scene.to_desc(...), possibly edited by the caller) instead of the scene's default one"""
        if not torch.cuda.is_available():
            raise SdxError("seqdex_amd needs a ROCm GPU (gfx950); there is no CPU fallback for the product path")
        self.lib = _abi.load_library()
        self.scene = scene or load_scene()
        self.device = torch.device(device)
        self.num_envs = int(num_envs)
        if desc is not None and desc_overrides:
            raise SdxError("SdxSim: pass either a ready `desc` or overrides for Scene.to_desc(), not both (%s would be ignored)"
                           % ", ".join(sorted(desc_overrides)))
        self._desc = desc if desc is not None else self.scene.to_desc(**desc_overrides)
        h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        rc = self.lib.sdx_create(C.byref(self._desc), self.num_envs, idx, C.c_uint64(seed), C.byref(h))
        if rc != 0:
            raise SdxError("sdx_create failed (%d): %s" % (rc, self.lib.sdx_last_error(None).decode()))
        self.h = h
        self.ring_wrapped = False     # set by ring_rows() when a ring it reads has wrapped (its rows are then in claim order, not serial order)
        self._tensors = {}
        for name, tid in _abi.T.items():
            self._tensors[name] = self._wrap(tid)

    def _wrap(self, tid):
        ptr, shape, ndim, dt = C.c_void_p(), (C.c_int64 * 4)(), C.c_int32(), C.c_int32()
        self._check(self.lib.sdx_tensor(self.h, tid, C.byref(ptr), shape, C.byref(ndim), C.byref(dt)))
        return wrap_device_pointer(ptr.value, [shape[i] for i in range(ndim.value)], dt.value, self.device)

    def _check(self, rc):
        if rc != 0:
            raise SdxError("libseqdex_hip error %d: %s" % (rc, self.lib.sdx_last_error(self.h).decode()))

    def tensor(self, name):
        return self._tensors[name]

    def __getattr__(self, name):
        t = self.__dict__.get("_tensors", {})
        if name.upper() in t:
            return t[name.upper()]
        raise AttributeError(name)

    def ring_rows(self, rows, keys, count):
        """the filled rows of one ring in SERIAL order: `rows` [slots, ...] and `keys` [slots] views of a ring and its key tensor
        (SDX_T_*_KEYS: step << 24 | env of the append), `count` appends so far.  The kernels claim ring slots with atomics, so the slot order
        is the hardware's; sorted by key the rows come out as a loop over steps and envs would have written them - the same on every
        run.  A ring that has WRAPPED (count > slots) keeps whichever rows landed last in each slot - which ones depends on the order the
        slots were claimed in, the serial-order guarantee is gone: `self.ring_wrapped` records it (callers that promise determinism
        assert it stayed False; size the run so that it does)."""
        if int(count) > rows.shape[0] and self is not None:
            if not self.ring_wrapped:      # said once per simulator: every consumer of the ring (terminal states, piles, T-value data sets) is affected
                import warnings
                warnings.warn("seqdex_amd: a terminal-state ring wrapped (%d appends into %d slots): its rows are in slot-claim order, not in serial "
                              "(step, env) order - the run is no longer bit-reproducible; harvest more often or size the run to the ring"
                              % (int(count), rows.shape[0]), RuntimeWarning, stacklevel=2)
            self.ring_wrapped = True
        k = int(min(int(count), rows.shape[0]))
        if k == 0:
            return rows[:0].clone()
        order = torch.argsort(keys[:k], stable=True)
        return rows[:k].index_select(0, order)

    # ------------------------------------------------------------------ C ABI calls
    def load_initial_states(self, piles):
        if torch.is_tensor(piles):
            piles = piles.detach().cpu().numpy()
        piles = np.ascontiguousarray(piles, dtype=np.float32)
        assert piles.ndim == 4 and piles.shape[0] == 8 and piles.shape[2:] == (132, 13), piles.shape
        self._check(self.lib.sdx_load_initial_states(self.h, piles.ctypes.data_as(C.c_void_p), piles.shape[1]))

    def set_tvalue_weights(self, state_dict_or_flat):
        if isinstance(state_dict_or_flat, dict):
            parts = []
            for n in ["linear1", "linear2", "linear3", "output_layer"]:
                parts.append(np.asarray(state_dict_or_flat[n + ".weight" if n + ".weight" in state_dict_or_flat
                                                           else n + "_weight"], dtype=np.float32).ravel())
                parts.append(np.asarray(state_dict_or_flat[n + ".bias" if n + ".bias" in state_dict_or_flat
                                                           else n + "_bias"], dtype=np.float32).ravel())
            flat = np.concatenate(parts)
        else:
            flat = np.ascontiguousarray(state_dict_or_flat, dtype=np.float32)
        assert flat.size == _abi.TV_PARAMS
        self._check(self.lib.sdx_set_tvalue_weights(self.h, flat.ctypes.data_as(C.c_void_p), flat.size))

    def set_retri_tvalue_weights(self, state_dict_or_flat):
        """BlockAssemblySearch: RetriGraspTValue(650, 2) parameters (state_dict with linear1/2/3 + output_layer, or the flat packing)"""
        if isinstance(state_dict_or_flat, dict):
            parts = []
            for n in ["linear1", "linear2", "linear3", "output_layer"]:
                parts.append(np.asarray(state_dict_or_flat[n + ".weight"], dtype=np.float32).ravel())
                parts.append(np.asarray(state_dict_or_flat[n + ".bias"], dtype=np.float32).ravel())
            flat = np.concatenate(parts)
        else:
            flat = np.ascontiguousarray(state_dict_or_flat, dtype=np.float32)
        assert flat.size == _abi.RETRI_TV_PARAMS, flat.size
        self._check(self.lib.sdx_set_retri_tvalue_weights(self.h, flat.ctypes.data_as(C.c_void_p), flat.size))

    def _act_ptr(self, actions):
        assert actions.is_cuda and actions.dtype == torch.float32 and actions.is_contiguous()
        assert actions.shape == (self.num_envs, _abi.NUM_ACTIONS)
        return C.c_void_p(actions.data_ptr())

    def step(self, actions):
        self._check(self.lib.sdx_step(self.h, self._act_ptr(actions), _stream_ptr(self.device)))

    def pre_physics(self, actions):
        self._check(self.lib.sdx_pre_physics(self.h, self._act_ptr(actions), _stream_ptr(self.device)))

    def simulate(self):
        self._check(self.lib.sdx_simulate(self.h, _stream_ptr(self.device)))

    def post_physics(self):
        self._check(self.lib.sdx_post_physics(self.h, _stream_ptr(self.device)))

    def compute_observations(self):
        self._check(self.lib.sdx_compute_observations(self.h, _stream_ptr(self.device)))

    def render_segmentation(self):
        """BlockAssemblySearch: gym.render_all_camera_sensors + pixel statistics -> SEG_IMAGE, SEG_PIXELS, EMERGENCE"""
        self._check(self.lib.sdx_render_segmentation(self.h, _stream_ptr(self.device)))

    def render_view(self, env_ids, camera, width, height, geometry="collision", depth=True, label=True, rgb=True, out=None):
        """view camera (include/seqdex.h sdx_render_view): images of the listed envs from the current ROOT / RB.
        env_ids: a sequence or an int32 tensor on the device (any subset, order, repeats); camera: a view.ViewCamera or one of
        "scene" / "overview" / "wrist"; geometry "collision" (what the physics collides) or "bounds" (the segmentation camera's boxes).
        Returns {"depth": f32 [n, H, W] (+inf: nothing hit), "label": i16 [n, H, W], "rgb": u8 [n, H, W, 3]} for the outputs asked for,
        device tensors; `out`: a dict returned earlier for the same shape, reused.  Stream-ordered, no synchronisation."""
        from .view import named_camera
        cam = named_camera(camera, self.scene, self._desc)
        if torch.is_tensor(env_ids):
            ids = env_ids
            assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.device.type == self.device.type, (ids.dtype, ids.device)
        else:
            ids = torch.as_tensor(list(env_ids), dtype=torch.int32).to(self.device)
        n, w, h = int(ids.numel()), int(width), int(height)
        spec = {"depth": (depth, (n, h, w), torch.float32), "label": (label, (n, h, w), torch.int16), "rgb": (rgb, (n, h, w, 3), torch.uint8)}
        res, ptr = {}, {}
        for k, (on, shape, dt) in spec.items():
            ptr[k] = None
            if not on:
                continue
            t = out.get(k) if out else None
            if t is None or tuple(t.shape) != shape or t.dtype != dt or t.device.type != self.device.type or not t.is_contiguous():
                t = torch.empty(shape, dtype=dt, device=self.device)
            res[k], ptr[k] = t, C.c_void_p(t.data_ptr())
        desc = cam.to_desc(w, h, geometry)
        stream = _stream_ptr(self.device) if self.device.type == "cuda" else None
        self._check(self.lib.sdx_render_view(self.h, C.byref(desc), C.c_void_p(ids.data_ptr()), n, ptr["depth"], ptr["label"], ptr["rgb"], stream))
        res["_ids"] = ids                     # (keeps the id tensor alive until the caller drops the result)
        return res

    def refresh_kinematics(self):
        self._check(self.lib.sdx_refresh_kinematics(self.h, _stream_ptr(self.device)))

    def reset_idx(self, env_mask, pile_choice=None):
        assert env_mask.is_cuda and env_mask.dtype == torch.uint8 and env_mask.numel() == self.num_envs
        pc = C.c_void_p(0)
        if pile_choice is not None:
            assert pile_choice.is_cuda and pile_choice.dtype == torch.int32 and pile_choice.numel() == self.num_envs
            pc = C.c_void_p(pile_choice.data_ptr())
        self._check(self.lib.sdx_reset_idx(self.h, C.c_void_p(env_mask.data_ptr()), pc, _stream_ptr(self.device)))

    def set_indexed(self, name, src, actor_ids):
        """gym.set_{actor_root_state,dof_state,dof_position_target}_tensor_indexed: name in ROOT / DOF / TARGETS, src the full-size
        tensor (the library's own view after in-place edits, or a tensor of the caller's), actor_ids int32 sim-domain actor indices"""
        assert name in ("ROOT", "DOF", "TARGETS"), name
        own = self._tensors[name]
        assert src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.numel() == own.numel(), (src.shape, own.shape)
        assert actor_ids.is_cuda and actor_ids.dtype == torch.int32 and actor_ids.is_contiguous()
        self._check(self.lib.sdx_set_indexed(self.h, _abi.T[name], C.c_void_p(src.data_ptr()), C.c_void_p(actor_ids.data_ptr()),
                                             int(actor_ids.numel()), _stream_ptr(self.device)))

    def set_randomization(self, spec):
        """domain randomization (include/seqdex.h sdx_set_randomization): `spec` = a task YAML's
        randomization_params mapping, a ready domain_randomization.DrDesc, or None (off: the physics returns to the scene constants).
        On: the first randomization is sampled on the device at once.  Returns the parse report (None for a DrDesc / None)."""
        from . import domain_randomization as dr
        report = None
        if spec is None:
            desc = None
        elif isinstance(spec, dr.DrDesc):
            desc = spec
        else:
            desc, report = dr.parse(spec)
        self._dr_desc = desc                  # (kept alive for the call)
        ptr = C.cast(C.pointer(desc), C.c_void_p) if desc is not None else None
        stream = _stream_ptr(self.device) if self.device.type == "cuda" else None
        self._check(self.lib.sdx_set_randomization(self.h, ptr, stream))
        return report

    def set_noise(self, spec=None, observations=None, actions=None):
        """observation / action noise (include/seqdex.h sdx_set_noise).  `spec` = a task YAML's
        randomization_params mapping (its `observations` / `actions` blocks are applied), or ready _abi.NoiseAttr blocks through the
        keywords; a side that is None is off, set_noise() turns both off.  Randomization must be on (set_randomization first; an
        identity_desc() is enough).  Returns the parse report of the mapping (None for ready blocks)."""
        from . import domain_randomization as dr
        report = None
        if spec is not None:
            if observations is not None or actions is not None:
                raise ValueError("set_noise: pass either the randomization_params mapping or ready blocks, not both")
            observations, actions, report = dr.parse_noise(spec)
        self._noise = (observations, actions)     # (kept alive for the call)
        ptr = [C.byref(a) if a is not None else None for a in self._noise]
        self._check(self.lib.sdx_set_noise(self.h, ptr[0], ptr[1], self._stream_or_none()))
        return report

    # ------------------------------------------------------------------ external wrenches (include/seqdex.h)
    def _wrench_tensor(self, t, what, shape):
        if t is None:
            return None
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() \
                or t.device.type != self.device.type or (t.device.type == "cuda" and t.device.index not in (None, self.device.index or 0)):
            raise ValueError("%s: expected a contiguous float32 tensor of shape %s on %s, got %s" % (
                what, shape, self.device, "%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__))
        return t

    def apply_rigid_body_forces(self, forces=None, torques=None, space="env"):
        """gym.apply_rigid_body_force_tensors: forces / torques float32 [N, BODIES, 3] indexed like RB (either may be None) act on the NEXT
        physics launch (simulate() or step()) only; at the centre of mass, in the env's axes ("env") or the body's ("local", rotated once
        with the start-of-step orientation).  A second call before that launch replaces the wrench, both None clears it.  Nothing is
        enqueued: the tensors are read by that launch, so they are kept referenced here until it has been enqueued."""
        spaces = {"env": _abi.SPACE_ENV, "local": _abi.SPACE_LOCAL}
        if space not in spaces and space not in spaces.values():
            raise ValueError("apply_rigid_body_forces: space must be 'env' or 'local', got %r" % (space,))
        shape = (self.num_envs, _abi.BODIES, 3)
        f = self._wrench_tensor(forces, "apply_rigid_body_forces: forces", shape)
        t = self._wrench_tensor(torques, "apply_rigid_body_forces: torques", shape)
        self._wrench = (f, t)
        self._check(self.lib.sdx_apply_rigid_body_forces(self.h, C.c_void_p(f.data_ptr()) if f is not None else None,
                                                         C.c_void_p(t.data_ptr()) if t is not None else None,
                                                         C.c_int32(spaces.get(space, space)), self._stream_or_none()))

    def set_force_perturbation(self, attr, rb_forces=None, prob=None):
        """random pushes on the target brick (sdx_set_force_perturbation): attr an _abi.ForcePerturbAttr, or None / force_scale <= 0 for
        off; rb_forces float32 [N, BODIES, 3] and prob float32 [N] are the CALLER'S tensors (the task's rb_forces / random_force_prob),
        read and written by every step() / pre_physics() / reset_idx() while on; they are kept referenced here.  Not part of a snapshot."""
        if attr is None:
            self._check(self.lib.sdx_set_force_perturbation(self.h, None, None, None, self._stream_or_none()))
            self._perturb = None
            return
        f = self._wrench_tensor(rb_forces, "set_force_perturbation: rb_forces", (self.num_envs, _abi.BODIES, 3))
        p = self._wrench_tensor(prob, "set_force_perturbation: prob", (self.num_envs,))
        self._check(self.lib.sdx_set_force_perturbation(self.h, C.byref(attr), C.c_void_p(f.data_ptr()) if f is not None else None,
                                                        C.c_void_p(p.data_ptr()) if p is not None else None, self._stream_or_none()))
        self._perturb = (attr, f, p) if attr.force_scale > 0 else None

    # ------------------------------------------------------------------ joint torques and dynamics (include/seqdex.h)
    def apply_dof_forces(self, forces=None, drive_off=None):
        """gym.set_dof_actuation_force_tensor with DOF_MODE_EFFORT per DOF: forces float32 [N, NDOF] (or None) are added to the joint
        torques of the NEXT physics launch (simulate() or step()) only, each clamped to its DOF's effort limit; drive_off: an int mask or
        an iterable of DOF indices whose PD drive is off in that launch.  A second call before the launch replaces both, no arguments
        clears them.  Nothing is enqueued: the tensor is read by that launch, so it is kept referenced here until it has been enqueued."""
        if drive_off is None:
            mask = 0
        elif isinstance(drive_off, (int, np.integer)):
            mask = int(drive_off)
        else:
            mask = 0
            for j in drive_off:
                if not 0 <= int(j) < _abi.NDOF:
                    raise ValueError("apply_dof_forces: drive_off names DOF %d outside [0, %d)" % (int(j), _abi.NDOF))
                mask |= 1 << int(j)
        if not 0 <= mask < 1 << 32:
            raise ValueError("apply_dof_forces: drive_off mask %r is no uint32" % (mask,))
        f = self._wrench_tensor(forces, "apply_dof_forces: forces", (self.num_envs, _abi.NDOF))
        self._dof_forces = f
        self._check(self.lib.sdx_apply_dof_forces(self.h, C.c_void_p(f.data_ptr()) if f is not None else None, C.c_uint32(mask),
                                                  self._stream_or_none()))

    def dof_dynamics(self, mass=True, bias=True, drive=True):
        """acquire_mass_matrix_tensor / the DOF force tensor, from the current DOF and TARGETS in one launch: DofDynamics(mass [N, NDOF,
        NDOF] = M(q) + armature, bias [N, NDOF] = C(q, qd) qd, drive [N, NDOF] = the clamped PD torque the next launch's first substep would
        apply); None for an output not asked for.  The tensors are allocated once and rewritten by every call.  Stream-ordered."""
        from .torque_control import DofDynamics
        n, nd = self.num_envs, _abi.NDOF
        if not hasattr(self, "_dyn"):
            self._dyn = {}
        out = []
        for name, on, shape in (("mass", mass, (n, nd, nd)), ("bias", bias, (n, nd)), ("drive", drive, (n, nd))):
            if on and name not in self._dyn:
                self._dyn[name] = torch.empty(shape, dtype=torch.float32, device=self.device)
            out.append(self._dyn[name] if on else None)
        self._check(self.lib.sdx_dof_dynamics(self.h, *[C.c_void_p(t.data_ptr()) if t is not None else None for t in out],
                                              self._stream_or_none()))
        return DofDynamics(*out)

    def osc_torques(self, dpose, gains, out=None, wrench=False):
        """operational-space (end-effector impedance) torques of the arm from the current DOF state in one launch (include/seqdex.h
        sdx_osc_torques).  dpose float32 [N, 6] (torque_control.pose_error); gains: a torque_control.OscGains or a
        ready _abi.OscAttr; out: float32 [N, NDOF] to write (default: a tensor allocated once and rewritten by every call).  Returns the
        torques, or (torques, wrench [N, 6]) with wrench=True; the row goes to apply_dof_forces(u, drive_off=0x7f) as it is.  Stream-ordered."""
        n = self.num_envs
        d = self._wrench_tensor(dpose, "osc_torques: dpose", (n, 6))
        if d is None:
            raise ValueError("osc_torques: dpose: expected a contiguous float32 tensor of shape %s on %s, got None" % ((n, 6), self.device))
        u = self._wrench_tensor(out, "osc_torques: out", (n, _abi.NDOF))
        if not hasattr(self, "_osc"):
            self._osc = {}
        if u is None:
            if "torques" not in self._osc:
                self._osc["torques"] = torch.empty((n, _abi.NDOF), dtype=torch.float32, device=self.device)
            u = self._osc["torques"]
        w = None
        if wrench:
            if "wrench" not in self._osc:
                self._osc["wrench"] = torch.empty((n, 6), dtype=torch.float32, device=self.device)
            w = self._osc["wrench"]
        attr = gains if isinstance(gains, _abi.OscAttr) else gains.to_attr()
        self._check(self.lib.sdx_osc_torques(self.h, C.byref(attr), C.c_void_p(d.data_ptr()), C.c_void_p(u.data_ptr()),
                                             C.c_void_p(w.data_ptr()) if w is not None else None, self._stream_or_none()))
        return (u, w) if wrench else u

    # ------------------------------------------------------------------ pose solver (include/seqdex.h)
    def solve_ik(self, base_pos=None, base_quat=None, tip_pos=None, params=None, q0=None, out=None):
        """arm and fingertip inverse kinematics in one launch (include/seqdex.h sdx_solve_ik): the joint angles that
        put the hand base at base_pos [N, 3] / base_quat [N, 4] (xyzw, as a row of RB) and the four fingertips at tip_pos [N, 4, 3], env
        frame, float32.  params: an ik.IkParams (default: all five tasks) or a ready _abi.IkAttr; a target may be None when params does
        not select its task.  q0 float32 [N, NDOF]: the start (None: the positions of DOF); out: float32 [N, NDOF] to write, q0 itself is
        allowed (default: a tensor allocated once and rewritten by every call).  Returns ik.IkSolution(q, err [N, 6], converged bool
        [N, 5], iters int32 [N, 5]); err, converged and iters are rewritten by every call.  Reads nothing but DOF (when q0 is None) and
        the limits; writes no tensor of the simulator.  Stream-ordered."""
        from .ik import IkParams, IkSolution
        n, nd = self.num_envs, _abi.NDOF
        attr = params if isinstance(params, _abi.IkAttr) else (IkParams() if params is None else params).to_attr()
        bp = self._wrench_tensor(base_pos, "solve_ik: base_pos", (n, 3))
        bq = self._wrench_tensor(base_quat, "solve_ik: base_quat", (n, 4))
        tp = self._wrench_tensor(tip_pos, "solve_ik: tip_pos", (n, 4, 3))
        if (attr.task_mask & 1) and (bp is None or bq is None):
            raise ValueError("solve_ik: %s: the hand-base task is selected, expected a contiguous float32 tensor on %s, got None" % (
                "base_pos" if bp is None else "base_quat", self.device))
        if (attr.task_mask & 0x1e) and tp is None:
            raise ValueError("solve_ik: tip_pos: a fingertip task is selected, expected a contiguous float32 tensor of shape %s on %s, got None" % (
                (n, 4, 3), self.device))
        start = self._wrench_tensor(q0, "solve_ik: q0", (n, nd))
        q = self._wrench_tensor(out, "solve_ik: out", (n, nd))
        if not hasattr(self, "_ik"):
            self._ik = {"q": torch.empty((n, nd), dtype=torch.float32, device=self.device),
                        "err": torch.empty((n, 6), dtype=torch.float32, device=self.device),
                        "info": torch.empty((n, 6), dtype=torch.int32, device=self.device)}
        if q is None:
            q = self._ik["q"]
        err, info = self._ik["err"], self._ik["info"]
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
        self._check(self.lib.sdx_solve_ik(self.h, C.byref(attr), P(start), P(bp), P(bq), P(tp), P(q), P(err), P(info), self._stream_or_none()))
        bits = torch.arange(5, dtype=torch.int32, device=self.device)
        return IkSolution(q, err, ((info[:, 0:1] >> bits) & 1).bool(), info[:, 1:])

    # ------------------------------------------------------------------ contact report (include/seqdex.h)
    def contact_report(self, enable=True):
        """gym.get_env_rigid_contacts on the device: allocates a contact_report.ContactReport (count, body, key, point, normal, force,
        separation of every contact of a step's last solve), arms it and returns it; while armed every simulate() / step() rewrites it
        on its stream and changes nothing else.  A second call returns the armed report.  enable=False disarms and drops it (returns
        None); close() disarms too.  Not part of a snapshot."""
        from .contact_report import ContactReport
        rep = getattr(self, "_contact_report", None)
        if not enable:
            if getattr(self, "h", None) is not None and self.h.value:
                self._check(self.lib.sdx_set_contact_report(self.h, None, self._stream_or_none()))
            self._contact_report = None
            return None
        if rep is None:
            rep = ContactReport(self)
            self._check(self.lib.sdx_set_contact_report(self.h, C.byref(rep.struct), self._stream_or_none()))
            self._contact_report = rep
        return rep

    # ------------------------------------------------------------------ sim snapshots (include/seqdex.h sdx_state_*)
    def _stream_or_none(self):
        return _stream_ptr(self.device) if self.device.type == "cuda" else None

    def env_class(self, env):
        """the class of an env: a saved state may only be put into an env of the class it came from (env & 7 = the target brick; InsertSim:
        additionally env % 3 = the base plate)"""
        e = int(env)
        var3 = self._desc.static_var_slot >= 0 or self._desc.task_kind == _abi.TASK_INSERT
        return (e & 7) + (8 * (e % 3) if var3 else 0)

    def same_class_envs(self, env):
        """the envs of this simulator that the state of `env` may be restored or cloned into (`env` itself included)"""
        if not 0 <= int(env) < self.num_envs:
            raise ValueError("same_class_envs: env %d outside [0, %d)" % (int(env), self.num_envs))
        c = self.env_class(env)
        return [e for e in range(self.num_envs) if self.env_class(e) == c]

    def _ids(self, ids, what, limit=None, unique=False):
        """an id list for a snapshot call -> (int32 device tensor, host list or None).  Host sequences are validated here (ValueError);
        device tensors go through unchecked (the kernel skips and counts bad entries)"""
        if torch.is_tensor(ids):
            assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.device.type == self.device.type, (what, ids.dtype, ids.device)
            return ids, None
        host = [int(i) for i in ids]
        if limit is not None and any(i < 0 or i >= limit for i in host):
            raise ValueError("%s: an index lies outside [0, %d): %s" % (what, limit, host))
        if unique and len(set(host)) != len(host):
            raise ValueError("%s: entries must be unique: %s" % (what, host))
        return torch.as_tensor(host, dtype=torch.int32).to(self.device), host

    def snapshot(self, rows=None):
        """device memory for `rows` env states (default: one per env) of this simulator's layout: a SimState"""
        return SimState(self, self.num_envs if rows is None else int(rows))

    def clone_envs(self, src, dst):
        """the state of env src[i] -> env dst[i] on the device (a source may repeat: fan-out).  Destinations must be unique, of their
        source's class and not sources themselves; host lists are checked (ValueError), device int32 tensors are not (bad entries are
        skipped and counted, state_stats())"""
        s, hs = self._ids(src, "clone_envs: src", self.num_envs)
        d, hd = self._ids(dst, "clone_envs: dst", self.num_envs, unique=True)
        if int(s.numel()) != int(d.numel()):
            raise ValueError("clone_envs: %d sources for %d destinations" % (int(s.numel()), int(d.numel())))
        if hs is not None and hd is not None:
            if set(hs) & set(hd):
                raise ValueError("clone_envs: envs %s are both a source and a destination" % sorted(set(hs) & set(hd)))
            bad = [(a, b) for a, b in zip(hs, hd) if self.env_class(a) != self.env_class(b)]
            if bad:
                raise ValueError("clone_envs: (src, dst) pairs of different env classes: %s" % bad)
        self._check(self.lib.sdx_state_clone(self.h, C.c_void_p(s.data_ptr()), C.c_void_p(d.data_ptr()), C.c_int32(int(s.numel())),
                                             self._stream_or_none()))
        self._clone_ids = (s, d)              # (keeps the id tensors alive until the next call)

    def state_stats(self):
        """entries the snapshot kernels skipped since create: [out of range, class mismatch, restore of a row never saved].  Blocking."""
        out = (C.c_int32 * 3)()
        self._check(self.lib.sdx_state_stats(self.h, out))
        return [int(v) for v in out]

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            if getattr(self, "_contact_report", None) is not None:
                self.contact_report(False)
            self._tensors.clear()
            self.lib.sdx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
