"""The contact report (include/seqdex.h sdx_contact_report / sdx_contact_wrenches): per-contact tensors of a step's
last solve and the per-body contact wrenches reduced from them, all on the device.

    rep = sim.contact_report()            # allocates, arms; every simulate() / step() now rewrites rep's tensors
    sim.step(actions)
    tips = fingertip_bodies(sim.scene)
    net = rep.net_wrenches()              # [N, BODIES, 6]: net contact force and torque on every row of RB
    fm = rep.pair_forces(tips, [target_row, -1])     # [N, 4, 2, 3]: force on each fingertip from the target brick / the static world
    on_target = (fm[:, :, 0].abs().sum(-1) > 0)      # "is the fingertip on the target brick?"

torch is plumbing here (the tensors and their pointers); the arithmetic is in libseqdex_hip.so."""
import collections
import ctypes as C

import torch

from . import _abi

MAX_CONTACTS = _abi.MAX_CONTACTS
NF, NSMAX, NT = _abi.NFREE, _abi.MAX_STATIC, 512        # free bricks, static slots of the pair enumeration, lanes of k_physics
N_BRICK_STATIC, N_BRICK_BRICK = NF * NSMAX, NF * (NF - 1) // 2
KIND_BRICK_STATIC, KIND_BRICK_BRICK, KIND_RBOX_BRICK, KIND_RBOX_STATIC = 0, 1, 2, 3

DecodedKeys = collections.namedtuple("DecodedKeys", "kind a b box_pair direction sample")


def decode_key(key):
    """the identity keys of a report (or of WARM_KEYS: the age nibble is ignored), any shape, -> DecodedKeys of int64 tensors of that shape:
      kind       KIND_BRICK_STATIC, KIND_BRICK_BRICK, KIND_RBOX_BRICK or KIND_RBOX_STATIC: what the two bodies of the candidate pair are
      a          the first body of the pair: a free brick (kinds 0, 1) or a robot box (kinds 2, 3; its link is scene rbox_link[a])
      b          the second: a static slot (kinds 0, 3) or a free brick (kinds 1, 2)
      box_pair   index of the pair of boxes inside the two bodies' compounds
      direction  0: the contact's side a is the pair's first body (its box is sampled against the second's); 1: the sides are swapped
      sample     which of the box's sample points
    A key is (rank of the body pair << 9 | box pair) << 6 | direction << 5 | sample with rank = lane x 16 + turn of the broadphase lane that
    tests the pair; the pair's place in the enumeration [brick x static slot | brick x brick, lower triangle | robot box x (brick, static
    slot)] is turn x 512 + lane."""
    k = key.to(torch.int64) & 0x0FFFFFFF
    rank, bp, d, smp = k >> 15, (k >> 6) & 0x1FF, (k >> 5) & 1, k & 31
    e = (rank % 16) * NT + rank // 16
    # brick x brick: e - N_BRICK_STATIC -> (i, j <= i) of the row-major lower triangle = bricks (j, i + 1)
    t = (e - N_BRICK_STATIC).clamp(min=0)
    i = ((torch.sqrt(8.0 * t.to(torch.float64) + 1.0) - 1.0) * 0.5).to(torch.int64)
    i = i - (i * (i + 1) // 2 > t).to(torch.int64)
    i = i + ((i + 1) * (i + 2) // 2 <= t).to(torch.int64)
    j = t - i * (i + 1) // 2
    r = (e - N_BRICK_STATIC - N_BRICK_BRICK).clamp(min=0)
    per = NF + NSMAX
    rbox, u = r // per, r % per
    is_bs, is_bb = e < N_BRICK_STATIC, (e >= N_BRICK_STATIC) & (e < N_BRICK_STATIC + N_BRICK_BRICK)
    kind = torch.where(is_bs, KIND_BRICK_STATIC, torch.where(is_bb, KIND_BRICK_BRICK, torch.where(u < NF, KIND_RBOX_BRICK, KIND_RBOX_STATIC)))
    a = torch.where(is_bs, e // NSMAX, torch.where(is_bb, j, rbox))
    b = torch.where(is_bs, e % NSMAX, torch.where(is_bb, i + 1, torch.where(u < NF, u, u - NF)))
    return DecodedKeys(kind, a, b, bp, d, smp)


def fingertip_bodies(scene):
    """rows of RB of the four fingertips (index, middle, ring, thumb): the sensor bodies of the Allegro force sensors"""
    return [int(b) for b in scene.fingertip_bodies]


class ContactReport:
    """The seven tensors of a contact report, owned here and written by the simulator's physics launches while armed
    (SdxSim.contact_report()).  Per env e the first count[e] columns are the contacts of the step's last solve, in the solver's order:
      count [N] i32;  body [N, 2, M] i32 (side a, side b: row of RB, -1 = the static world);  key [N, M] i32 (the bits of the u32 identity;
      decode_key());  point, normal, force [N, 3, M] f32 (env frame; force acts on side a, side b receives the negative);  separation [N, M]
      f32;  M = MAX_CONTACTS.  Columns at or beyond count[e] hold whatever they held before (valid_mask())."""

    FIELDS = ("count", "body", "key", "point", "normal", "force", "separation")

    def __init__(self, sim):
        n, m, dev = sim.num_envs, MAX_CONTACTS, sim.device
        self.sim = sim
        self.count = torch.zeros(n, dtype=torch.int32, device=dev)
        self.body = torch.full((n, 2, m), -1, dtype=torch.int32, device=dev)
        self.key = torch.zeros((n, m), dtype=torch.int32, device=dev)
        self.point = torch.zeros((n, 3, m), dtype=torch.float32, device=dev)
        self.normal = torch.zeros((n, 3, m), dtype=torch.float32, device=dev)
        self.force = torch.zeros((n, 3, m), dtype=torch.float32, device=dev)
        self.separation = torch.zeros((n, m), dtype=torch.float32, device=dev)
        self.struct = _abi.ContactReportStruct(*[getattr(self, f).data_ptr() for f in self.FIELDS])
        self._keep = None

    def valid_mask(self):
        """[N, MAX_CONTACTS] bool: column c of env e is a contact of the report"""
        return torch.arange(MAX_CONTACTS, device=self.count.device)[None, :] < self.count.clamp(0, MAX_CONTACTS)[:, None]

    def _out(self, out, shape, what):
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.count.device)
        if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != self.count.device:
            raise ValueError("%s: out must be a contiguous float32 tensor of shape %s on %s" % (what, shape, self.count.device))
        return out

    def net_wrenches(self, out=None):
        """[N, BODIES, 6]: per row of RB the sum of the contact forces on the body and their torque about the position of its RB row at
        the time of the call (acquire_net_contact_force_tensor for every body, plus the force-sensor torque).  One launch, deterministic."""
        sim = self.sim
        out = self._out(out, (sim.num_envs, _abi.BODIES, 6), "net_wrenches")
        sim._check(sim.lib.sdx_contact_wrenches(sim.h, C.byref(self.struct), C.c_void_p(out.data_ptr()), None, None, sim._stream_or_none()))
        return out

    def pair_forces(self, sensor_bodies, filter_bodies, out=None):
        """[N, len(sensor_bodies), len(filter_bodies), 3]: the contact force on sensor body s from filter body f (rows of RB; a filter of
        -1 is the static world) - IsaacLab's ContactSensor.force_matrix_w.  At most 32 of each."""
        sim = self.sim
        s, f = [int(v) for v in sensor_bodies], [int(v) for v in filter_bodies]
        if len(s) > 32 or len(f) > 32:
            raise ValueError("pair_forces: at most 32 sensor and 32 filter bodies (got %d, %d)" % (len(s), len(f)))
        pairs = _abi.ContactPairs(len(s), len(f))
        pairs.sensor_body[:len(s)] = s
        pairs.filter_body[:len(f)] = f
        out = self._out(out, (sim.num_envs, len(s), len(f), 3), "pair_forces")
        sim._check(sim.lib.sdx_contact_wrenches(sim.h, C.byref(self.struct), None, C.byref(pairs), C.c_void_p(out.data_ptr()),
                                                sim._stream_or_none()))
        return out
