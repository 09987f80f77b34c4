"""Shared bodies of the contact-report tests (include/seqdex.h sdx_set_contact_report / sdx_contact_wrenches):
tests/test_contact_report.py runs them on the emulated simulator (tests/hipemu), tests/test_gpu_contact_report.py on the GPU.  A `backend`
is (make, dev): make(n, **desc) builds a simulator, dev(tensor) moves a host tensor to where its tensors live.

What the report is held to: the C oracle contact by contact (identities, bodies, geometry, impulses), SDX_T_CONTACT (the links' net
forces), Newton's second law on every free brick, and a float64 numpy reduction for the reducer.  Bars that are measured are twice the
largest difference seen on the emulator and on an MI355X (profiles/contact_report_parity.txt); every case prints its figures before it
asserts."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import torch

from helpers import force_perturb_restatement as fr
from seqdex_amd import _abi
from seqdex_amd import contact_report as cr
from seqdex_amd import domain_randomization as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NB, B0, A0, NF, NL, ND, M = _abi.BODIES, _abi.BODY_BRICK0, _abi.ACTOR_BRICK0, _abi.NFREE, _abi.NLINK, _abi.NDOF, _abi.MAX_CONTACTS
NEVER = 10 ** 9
EPS = 2.0 ** -24
FIELDS = cr.ContactReport.FIELDS

# ---- measured bars of case_oracle_parity and case_newton: twice the largest difference seen, emulator and MI355X (profiles/contact_report_parity.txt)
POINT_CEILING = 2e-6                 # m: tests/helpers/contact_sets.DELTA, what fma contraction does to a coordinate
IMPULSE_CEILING = (2e-2, 2e-5)       # rtol, atol (N s) of tests/test_gpu_physics_contact_parity.py; forces: divided by h
POINT_BAR = 6.4e-7                   # m, points and separations: measured 3.0e-7 / 3.2e-7 (emulator), 2.4e-7 / 2.4e-7 (MI355X)
# components of a unit vector; no ceiling is known.  Measured 2.7e-4 (emulator), 1.41e-2 (MI355X: one contact of env 7, step 0; every other
# env stays below 7e-4).  The normal of a sample beside an edge or a corner is a difference of coordinates divided by its length, the
# separation: a coordinate that differs by 1e-7 m turns it by 1e-7 / |separation|
NORMAL_BAR = 2.9e-2
K_IMPULSE = 0.15                     # in units of the impulse ceiling: measured 0.073 (emulator), 0.043 (MI355X)
NEWTON_BAR = 1.4e-7                  # N s: measured 6.7e-8 (emulator), 7.0e-8 (MI355X), on impulses of up to 3.3e-2 N s


def host(t):
    return t.detach().cpu().numpy().copy()


def golden_state(golden_dir):
    return np.load(os.path.join(golden_dir, "P1_settled_state.npz"))


def load_state(s, dev, root, dof, tg):
    s.ROOT.copy_(dev(torch.from_numpy(np.ascontiguousarray(root, f32).reshape(-1, 13))))
    s.DOF.copy_(dev(torch.from_numpy(np.ascontiguousarray(dof, f32).reshape(-1, 2))))
    s.TARGETS.copy_(dev(torch.from_numpy(np.ascontiguousarray(tg, f32))))


def report_host(rep):
    """host copies of the seven tensors; key as uint32"""
    r = {k: host(getattr(rep, k)) for k in FIELDS}
    r["key"] = r["key"].view(np.uint32)
    return r


def identities(keys):
    """decode_key() of a 1-d key array as the tuples of tests/helpers/contact_keys.py"""
    d = cr.decode_key(torch.from_numpy(np.ascontiguousarray(keys).view(np.int32)))
    kind, a, b, bp, di, smp = [v.numpy() for v in d]
    na = {cr.KIND_BRICK_STATIC: "brick", cr.KIND_BRICK_BRICK: "brick", cr.KIND_RBOX_BRICK: "rbox", cr.KIND_RBOX_STATIC: "rbox"}
    nb = {cr.KIND_BRICK_STATIC: "static", cr.KIND_BRICK_BRICK: "brick", cr.KIND_RBOX_BRICK: "brick", cr.KIND_RBOX_STATIC: "static"}
    return [((na[int(kind[i])], int(a[i])), (nb[int(kind[i])], int(b[i])), int(bp[i]), int(di[i]), int(smp[i])) for i in range(len(keys))]


def reorder_bound(count, terms):
    """what a reordered float32 sum of `terms` [..., k] may differ by: count x 2^-24 x sum |term|"""
    return count * EPS * np.abs(terms).sum(-1)


def link_sums(r, e):
    """float64 sums of +-force over the report of env e for the 24 links, and sum |force|: [24, 3] each"""
    c = int(r["count"][e])
    F = r["force"][e, :, :c].astype(np.float64)
    tot, mag = np.zeros((NL, 3)), np.zeros((NL, 3))
    for side, sg in ((0, 1.0), (1, -1.0)):
        b = r["body"][e, side, :c]
        for k in range(NL):
            sel = b == k
            tot[k] += sg * F[:, sel].sum(1)
            mag[k] += np.abs(F[:, sel]).sum(1)
    return tot, mag


# ------------------------------------------------------------------------------------------------------------------ 1. ABI
def case_abi(backend):
    make, dev = backend
    src = ('#include <stdio.h>\n#include "seqdex.h"\nint main(){printf("%zu %zu %d %d\\n", sizeof(sdx_contact_report), sizeof(sdx_contact_pairs), '
           'SDX_ABI_VERSION, SDX_MAX_CONTACTS);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        a, b, abi, maxc = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert a == C.sizeof(_abi.ContactReportStruct) == 56 and b == C.sizeof(_abi.ContactPairs) == 264
    assert abi == _abi.SDX_ABI_VERSION == 8 and len(_abi.T) == 56 and maxc == _abi.MAX_CONTACTS == 1536      # no tensor id, no version bump
    assert "sdx_set_contact_report" in _abi.SDX_EXPORTS and "sdx_contact_wrenches" in _abi.SDX_EXPORTS
    s = make(2, seed=22)
    try:
        lib, h = s.lib, s.h
        assert hasattr(lib, "sdx_set_contact_report") and hasattr(lib, "sdx_contact_wrenches")
        rep = cr.ContactReport(s)
        net = dev(torch.zeros(2, NB, 6))
        pf = dev(torch.zeros(2, 2, 2, 3))
        netp, pfp = C.c_void_p(net.data_ptr()), C.c_void_p(pf.data_ptr())

        def pairs(ns=2, nf=2, sensor=(3, 4), filt=(B0, -1)):
            p = _abi.ContactPairs(ns, nf)
            p.sensor_body[:len(sensor)] = list(sensor)
            p.filter_body[:len(filt)] = list(filt)
            return p

        def invalid(rc, word):
            msg = lib.sdx_last_error(h)
            assert rc == -1 and msg and word in msg, (rc, msg, word)

        def struct(**null):
            st = _abi.ContactReportStruct.from_buffer_copy(rep.struct)
            for k in null:
                setattr(st, k, None)
            return st

        invalid(lib.sdx_set_contact_report(h, C.byref(struct(count=1)), None), b"sdx_set_contact_report: report->count is NULL")
        invalid(lib.sdx_contact_wrenches(h, None, netp, None, None, None), b"report is NULL")
        for k in ("count", "body", "point", "force"):
            invalid(lib.sdx_contact_wrenches(h, C.byref(struct(**{k: 1})), netp, None, None, None), b"count, body, point and force")
        invalid(lib.sdx_contact_wrenches(h, C.byref(rep.struct), None, None, None, None), b"both NULL")
        invalid(lib.sdx_contact_wrenches(h, C.byref(rep.struct), None, C.byref(pairs()), None, None), b"both NULL")
        invalid(lib.sdx_contact_wrenches(h, C.byref(rep.struct), netp, None, pfp, None), b"pair_dev without pairs")
        for kw in (dict(ns=33), dict(ns=-1), dict(nf=33), dict(nf=-1)):
            invalid(lib.sdx_contact_wrenches(h, C.byref(rep.struct), None, C.byref(pairs(**kw)), pfp, None), b"0..32")
        for bad in (-1, NB, 1 << 20):
            invalid(lib.sdx_contact_wrenches(h, C.byref(rep.struct), None, C.byref(pairs(sensor=(3, bad))), pfp, None), b"sensor body")
        # what is allowed: NULL key / normal / separation, a report armed with count alone, disarming twice, both outputs at once
        assert lib.sdx_contact_wrenches(h, C.byref(struct(key=1, normal=1, separation=1)), netp, C.byref(pairs()), pfp, None) == 0
        only = _abi.ContactReportStruct(rep.count.data_ptr())
        assert lib.sdx_set_contact_report(h, C.byref(only), None) == 0
        s.simulate()
        assert lib.sdx_set_contact_report(h, None, None) == 0 and lib.sdx_set_contact_report(h, None, None) == 0
        a1 = s.contact_report()
        assert s.contact_report() is a1 and s.contact_report(False) is None and s.contact_report() is not a1
        assert tuple(a1.valid_mask().shape) == (2, M) and len(cr.fingertip_bodies(s.scene)) == 4
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 2. armed changes nothing
STATE = ("ROOT", "DOF", "RB", "CONTACT", "NCONTACTS", "WARM_COUNT", "WARM_KEYS", "WARM_LAMBDA")


def case_armed_changes_nothing(backend, golden_dir, randomize, dof_force, steps=4):
    """the 8 golden piles, default two substeps, 4 steps with the report armed and without it: the state and the warm-start cache are equal
    bit for bit (randomize: the DR variants; dof_force: a pending sdx_apply_dof_forces row, so that the FORCE | REPORT variant runs).
    Then: the report is what the step says (count, keys), and after disarming a sentinel-filled report stays untouched."""
    make, dev = backend
    st = golden_state(golden_dir)
    n = st["root"].shape[0]
    u = dev(torch.from_numpy(np.random.default_rng(3).uniform(-0.2, 0.2, (n, ND)).astype(f32)))

    def run(armed):
        s = make(n, seed=22, warm_start=0.8)
        try:
            if randomize:
                s.set_randomization(dr.identity_desc(NEVER))
            load_state(s, dev, st["root"], st["dof"], st["targets"])
            rep = s.contact_report() if armed else None
            out = []
            for _ in range(steps):
                if dof_force:
                    s.apply_dof_forces(u)
                s.simulate()
                out.append({k: host(s.tensor(k)) for k in STATE})
            extra = None
            if armed:
                r = report_host(rep)
                assert (r["count"] == np.minimum(out[-1]["NCONTACTS"], M)).all() and (r["count"] == out[-1]["WARM_COUNT"]).all()
                assert int(r["count"].min()) > 500
                wk = out[-1]["WARM_KEYS"].view(np.uint32).reshape(n, -1)
                for e in range(n):
                    c = int(r["count"][e])
                    np.testing.assert_array_equal(r["key"][e, :c], wk[e, :c] & 0x0FFFFFFF)
                assert s.contact_report(False) is None
                for k in FIELDS:                                                  # (rep keeps the tensors alive)
                    getattr(rep, k).fill_(-7.0 if getattr(rep, k).dtype.is_floating_point else 0x5A5A5A5A)
                sentinel = report_host(rep)
                if dof_force:
                    s.apply_dof_forces(u)
                s.simulate()
                after = report_host(rep)
                for k in FIELDS:
                    np.testing.assert_array_equal(after[k], sentinel[k], err_msg="disarmed, %s" % k)
                extra = {k: host(s.tensor(k)) for k in STATE}
            return out, extra
        finally:
            s.close()

    plain, _ = run(False)
    armed, _ = run(True)
    assert int(plain[-1]["NCONTACTS"].min()) > 500
    for i in range(steps):
        for k in STATE:
            np.testing.assert_array_equal(armed[i][k].view(np.uint8), plain[i][k].view(np.uint8), err_msg="step %d %s" % (i, k))


# ------------------------------------------------------------------------------------------------------------------ 3. the oracle, contact by contact
def case_oracle_parity(backend, golden_dir, tag):
    """the 8 golden piles, one substep, warm start 0.8, two teacher-forced steps, as in tests/test_gpu_physics_contact_parity.py: the report
    against the oracle's contact list of the start state (tests/helpers/contact_sets.oracle_list, po.contacts) and its warm cache."""
    from oracle import physics_oracle as po
    from tests.helpers.contact_keys import decode_kernel
    from tests.helpers.contact_sets import DELTA, boundary_pairs, box_pair, decode_cache, decode_oracle, oracle_list
    make, dev = backend
    st = golden_state(golden_dir)
    n = st["root"].shape[0]
    s = make(n, seed=22, warm_start=0.8, substeps=1)
    try:
        desc, ns = s._desc, int(s._desc.n_static)
        h = float(desc.dt) / int(desc.substeps)
        rbl = [int(desc.rbox_link[i]) for i in range(int(desc.n_rbox))]
        root, dof, tg = st["root"].copy(), st["dof"].copy(), st["targets"].copy()
        o_warm = po.WarmState(n)
        rep = s.contact_report()
        worst = dict(point=0.0, sep=0.0, normal=0.0, impulse=0.0)
        rtol, atol = IMPULSE_CEILING

        def row_of(kind_index):        # an identity's body -> the row of SDX_T_RB the report names
            kind, i = kind_index
            return B0 + i if kind == "brick" else (rbl[i] if kind == "rbox" else -1)

        for it in range(2):
            load_state(s, dev, root, dof, tg)
            s.simulate()
            r = report_host(rep)
            wcount, nc = host(s.WARM_COUNT), host(s.NCONTACTS)
            wkey = host(s.WARM_KEYS).view(np.uint32).reshape(n, -1)
            np.testing.assert_array_equal(r["count"], wcount)
            np.testing.assert_array_equal(r["count"], np.minimum(nc, M))
            o_root, o_dof = root.copy(), dof.copy()
            po.simulate(desc, o_root, o_dof, tg, o_warm)
            for e in range(n):
                c = int(r["count"][e])
                np.testing.assert_array_equal(r["key"][e, :c], wkey[e, :c] & 0x0FFFFFFF)
                ids = identities(r["key"][e, :c])
                assert ids == [decode_kernel(k) for k in r["key"][e, :c]]          # the product's decode against the test helper's
                assert len(set(ids)) == c
                col = {k: i for i, k in enumerate(ids)}
                olist, total = oracle_list(desc, root[e], dof[e])
                ocon, _ = po.contacts(desc, root[e], dof[e])
                assert total == len(olist) == len(ocon) == int(o_warm.count[e])
                O = {k: i for i, (k, _) in enumerate(olist)}
                olam = decode_cache(o_warm.key[e], o_warm.lam[e], o_warm.count[e], lambda k: decode_oracle(k, ns))
                assert set(olam) == set(O)
                bp = boundary_pairs(desc, root[e], dof[e], desc.contact_offset, DELTA)
                assert sum(1 for k in O if box_pair(k) in bp) <= 0.05 * len(O), (it, e, len(bp))      # (from the oracle alone)
                diff = set(col) ^ set(O)
                stray = sorted(k for k in diff if box_pair(k) not in bp)
                assert not stray, ("contacts that differ outside the oracle's boundary pairs", stray[:6], len(stray))
                common = sorted(set(col) & set(O))
                gi, oi = np.array([col[k] for k in common]), np.array([O[k] for k in common])
                # sides: the pair's bodies, swapped where the direction bit is set (the box of side a is the one that is sampled)
                want = np.array([[row_of(k[1]), row_of(k[0])] if k[3] else [row_of(k[0]), row_of(k[1])] for k in common])
                np.testing.assert_array_equal(r["body"][e][:, gi].T, want)
                oa, ob = ocon[oi, 0].astype(int), ocon[oi, 1].astype(int)          # the oracle's own ids: brick i, NF + link, 255 = static
                o_rows = np.stack([np.where(oa < NF, B0 + oa, np.where(oa == 255, -1, oa - NF)), np.where(ob < NF, B0 + ob, np.where(ob == 255, -1, ob - NF))], 1)
                np.testing.assert_array_equal(r["body"][e][:, gi].T, o_rows)
                dp = float(np.abs(r["point"][e][:, gi].T - ocon[oi, 2:5]).max())
                dn = float(np.abs(r["normal"][e][:, gi].T - ocon[oi, 5:8]).max())
                ds = float(np.abs(r["separation"][e][gi] - ocon[oi, 8]).max())
                F, Nn = r["force"][e][:, gi].astype(np.float64), r["normal"][e][:, gi].astype(np.float64)
                lam = np.array([olam[k][1] for k in common], np.float64)           # [k, 3]
                fn = (F * Nn).sum(0)
                ft = np.sqrt(((F - fn * Nn) ** 2).sum(0))
                d0 = np.abs(fn * h - lam[:, 0]) / (atol + rtol * np.abs(lam[:, 0]))
                lt = np.sqrt(lam[:, 1] ** 2 + lam[:, 2] ** 2)
                d1 = np.abs(ft * h - lt) / (atol + rtol * lt)
                di = float(max(d0.max(), d1.max()))
                print("contact report parity [%s]: step %d env %d: contacts %d / %d, boundary pairs %d, excused %d, point %.2e m, separation %.2e m, "
                      "normal %.2e, impulses %.2e of the ceiling" % (tag, it, e, c, len(O), len(bp), len(diff), dp, ds, dn, di))
                worst = dict(point=max(worst["point"], dp), sep=max(worst["sep"], ds), normal=max(worst["normal"], dn), impulse=max(worst["impulse"], di))
            root, dof = o_root, o_dof                                              # teacher forcing
        print("contact report parity [%s]: largest differences: point %.3e m, separation %.3e m, normal %.3e, impulses %.3e of the ceiling "
              "(rtol %g, atol %g N s)" % (tag, worst["point"], worst["sep"], worst["normal"], worst["impulse"], rtol, atol))
        assert POINT_BAR <= POINT_CEILING and K_IMPULSE <= 1.0
        assert worst["point"] <= POINT_BAR and worst["sep"] <= POINT_BAR, worst
        assert worst["normal"] <= NORMAL_BAR, worst
        assert worst["impulse"] <= K_IMPULSE, worst
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 4. SDX_T_CONTACT
def hand_on_bricks_state(st, e=0):
    """the golden pile e with the fingers driven closed: after a few steps the hand presses on the bricks under it"""
    root, dof, tg = st["root"][e:e + 1].copy(), st["dof"][e:e + 1].copy(), st["targets"][e:e + 1].copy()
    tg[:, 7:] += 0.6
    return root, dof, tg


def case_contact_tensor(backend, golden_dir):
    """default two substeps; the 8 piles and a ninth env whose fingers close on the bricks, three steps: for every link the float64 sum of
    +-force over the report is the link's SDX_T_CONTACT row, within the rounding of a reordered float32 sum, count x 2^-24 x sum |force| per
    component."""
    make, dev = backend
    st = golden_state(golden_dir)
    xr, xd, xt = hand_on_bricks_state(st)
    root, dof, tg = np.concatenate([st["root"], xr]), np.concatenate([st["dof"], xd]), np.concatenate([st["targets"], xt])
    n = root.shape[0]
    s = make(n, seed=22, warm_start=0.8)
    try:
        load_state(s, dev, root, dof, tg)
        rep = s.contact_report()
        touched = np.zeros(n, int)
        for it in range(3):
            s.simulate()
            r = report_host(rep)
            con = host(s.CONTACT).reshape(n, NB, 3)
            assert not con[:, NL:].any()
            for e in range(n):
                tot, mag = link_sums(r, e)
                bound = int(r["count"][e]) * EPS * mag
                err = np.abs(tot - con[e, :NL])
                touched[e] = int((mag.sum(1) > 0).sum())
                print("contact report vs SDX_T_CONTACT: step %d env %d: count %d, links in contact %d, largest |force| %.3e, largest difference %.2e "
                      "(%.3f of its bound)" % (it, e, r["count"][e], touched[e], np.abs(con[e]).max(), err.max(),
                                               (err / np.maximum(bound, 1e-300))[mag > 0].max() if (mag > 0).any() else 0.0))
                assert (err <= bound).all(), (it, e, float(err.max()))
        assert touched[-1] >= 2 and (touched > 0).all(), touched                    # the hand touches bricks: in every pile, several links in the ninth env
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 5. Newton on the bricks
def case_newton(backend, golden_dir, tag):
    """one substep, no randomization: for every free brick m (v' - v) - m g h = h x the float64 sum of the report's forces on it, m the
    solver's mass (brick_mass, x seg_mass_scale on the target brick)."""
    make, dev = backend
    st = golden_state(golden_dir)
    n = st["root"].shape[0]
    s = make(n, seed=22, warm_start=0.8, substeps=1)
    try:
        d = s._desc
        h = float(d.dt) / int(d.substeps)
        g = np.array([float(d.gravity[i]) for i in range(3)])
        load_state(s, dev, st["root"], st["dof"], st["targets"])
        rep = s.contact_report()
        worst, longest = 0.0, 0
        for it in range(2):
            v0 = host(s.ROOT).reshape(n, -1, 13)[:, A0:A0 + NF, 7:10].astype(np.float64)
            s.simulate()
            v1 = host(s.ROOT).reshape(n, -1, 13)[:, A0:A0 + NF, 7:10].astype(np.float64)
            r = report_host(rep)
            for e in range(n):
                c = int(r["count"][e])
                F = r["force"][e, :, :c].astype(np.float64)
                tot, sides = np.zeros((NF, 3)), np.zeros(NF, int)
                for side, sg in ((0, 1.0), (1, -1.0)):
                    b = r["body"][e, side, :c]
                    sel = (b >= B0) & (b < B0 + NF)
                    np.add.at(tot, b[sel] - B0, sg * F[:, sel].T)
                    np.add.at(sides, b[sel] - B0, 1)
                m = np.array([float(d.brick_mass[d.brick_type[i]]) * (float(d.seg_mass_scale) if i == int(fr.target_brick(e)) else 1.0) for i in range(NF)])
                lhs = m[:, None] * (v1[e] - v0[e]) - m[:, None] * g[None, :] * h
                err = float(np.abs(lhs - h * tot).max())
                print("contact report, Newton [%s]: step %d env %d: count %d, longest brick list %d sides, largest impulse %.3e N s, largest difference "
                      "%.3e N s" % (tag, it, e, c, sides.max(), np.abs(h * tot).max(), err))
                worst, longest = max(worst, err), max(longest, int(sides.max()))
        print("contact report, Newton [%s]: largest difference %.3e N s" % (tag, worst))
        assert longest > 40, longest
        assert worst <= NEWTON_BAR, worst
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 6. the reducer
def numpy_wrenches(r, rb, e, sensors, filters):
    """float64 reduction of env e of a downloaded report: net [165, 6], pair [ns, nf, 3], and the sums of |term| behind each entry"""
    c = int(np.clip(r["count"][e], 0, M))
    F, P = r["force"][e, :, :c].astype(np.float64).T, r["point"][e, :, :c].astype(np.float64).T
    net, mag = np.zeros((NB, 6)), np.zeros((NB, 6))
    pair, pmag = np.zeros((len(sensors), len(filters), 3)), np.zeros((len(sensors), len(filters), 3))
    A, Bb = r["body"][e, 0, :c], r["body"][e, 1, :c]
    for i in range(c):
        for me, other, sg in ((A[i], Bb[i], 1.0), (Bb[i], A[i], -1.0)):
            if me < 0:
                continue
            arm = P[i] - rb[e, me, :3].astype(np.float64)
            net[me, :3] += sg * F[i]
            net[me, 3:] += np.cross(arm, sg * F[i])
            mag[me, :3] += np.abs(F[i])
            mag[me, 3:] += np.abs(arm[[1, 2, 0]] * F[i][[2, 0, 1]]) + np.abs(arm[[2, 0, 1]] * F[i][[1, 2, 0]])
            for si, sb in enumerate(sensors):
                for fi, fb in enumerate(filters):
                    if me == sb and other == fb:
                        pair[si, fi] += sg * F[i]
                        pmag[si, fi] += np.abs(F[i])
    return net, mag, pair, pmag


def case_reducer(backend, golden_dir):
    """N = 3, one substep, contact offset 1.4 cm (the recipe of test_capacity_rule_on_device): env 0 the golden pile 0 (1 515 contacts, the
    longest list the piles give), env 1 the same pile with every free brick lifted into free flight (count 0), env 2 the golden pile 1, whose
    first pass exceeds the capacity and whose list is rebuilt.  The report's columns beyond count are NaN / sentinels before the step."""
    make, dev = backend
    st = golden_state(golden_dir)
    pick = [0, 0, 1]
    root, dof, tg = st["root"][pick].copy(), st["dof"][pick].copy(), st["targets"][pick].copy()
    i = np.arange(NF)
    root[1, A0:A0 + NF, 0:3] = np.stack([(i % 9) * 0.3 - 1.2, (i // 9) * 0.3 - 1.05, np.full(NF, 3.0)], 1)     # a grid in the air, 0.3 m apart
    root[1, A0:A0 + NF, 7:13] = 0.0
    dof[1, 1, 0] -= 0.3                                                            # (the shoulder raised: at this offset the pile's hand pose is within reach of the floor)
    tg[1, 1] -= 0.3
    n = 3
    s = make(n, seed=22, warm_start=0.8, substeps=1, contact_offset=0.014)
    try:
        load_state(s, dev, root, dof, tg)
        rep = s.contact_report()
        for k in FIELDS[1:]:
            getattr(rep, k).fill_(float("nan") if getattr(rep, k).dtype.is_floating_point else 0x5A5A5A5A)
        s.simulate()
        r = report_host(rep)
        stats = host(s.CONTACT_STATS)
        print("contact report, reducer: counts %s, NCONTACTS %s, capacity statistics %s" % (r["count"].tolist(), host(s.NCONTACTS).tolist(), stats.tolist()))
        assert r["count"][0] > 1400 and r["count"][1] == 0 and 500 < r["count"][2] < 1000 and stats[2] == 1 and stats[1] == 0, (r["count"], stats)
        for e in range(n):                                                        # columns beyond count keep what they held
            c = int(r["count"][e])
            for k in ("point", "normal", "force"):
                assert np.isnan(r[k][e, :, c:]).all() and np.isfinite(r[k][e, :, :c]).all(), (e, k)
            assert np.isnan(r["separation"][e, c:]).all() and (r["key"][e, c:] == 0x5A5A5A5A).all() and (r["body"][e, :, c:] == 0x5A5A5A5A).all()
        tips = cr.fingertip_bodies(s.scene)
        sensors = tips + [int(s.scene.hand_base_body)]
        SENT = -12345.5
        nf = 3
        big_net = dev(torch.full((n * NB * 6 + 64,), SENT))
        big_pf = dev(torch.full((n * len(sensors) * nf * 3 + 64,), SENT))
        rb = host(s.RB).reshape(n, NB, 13)
        outs = []
        # one filter list per launch (the filters are the env's target brick, another brick, the static world: env e is checked in the launch with its own)
        for e in range(n):
            tb = int(fr.target_brick(e))
            # "one other brick": the brick that carries most contacts with the sensors in this env's report, if there is one
            c = int(r["count"][e])
            A, Bb = r["body"][e, 0, :c], r["body"][e, 1, :c]
            partner = np.concatenate([Bb[np.isin(A, sensors)], A[np.isin(Bb, sensors)]])
            partner = partner[(partner >= B0) & (partner != B0 + tb)]
            other = int(np.bincount(partner).argmax()) if len(partner) else B0 + (tb + 5) % NF
            filters = [B0 + tb, other, -1]
            net = rep.net_wrenches(out=big_net[:n * NB * 6].view(n, NB, 6))
            pf = rep.pair_forces(sensors, filters, out=big_pf[:n * len(sensors) * nf * 3].view(n, len(sensors), nf, 3))
            net_h, pf_h = host(net), host(pf)
            net2, pf2 = host(rep.net_wrenches()), host(rep.pair_forces(sensors, filters))
            np.testing.assert_array_equal(net_h.view(np.uint32), net2.view(np.uint32))          # two calls agree bit for bit
            np.testing.assert_array_equal(pf_h.view(np.uint32), pf2.view(np.uint32))
            assert (host(big_net)[n * NB * 6:] == f32(SENT)).all() and (host(big_pf)[n * len(sensors) * nf * 3:] == f32(SENT)).all()
            assert np.isfinite(net_h).all() and np.isfinite(pf_h).all()            # nothing of the NaN columns reaches an output
            ref_net, mag, ref_pf, pmag = numpy_wrenches(r, rb, e, sensors, filters)
            c = int(r["count"][e])
            # the torque terms are float32 products of a float32 difference: three roundings more per term than the sum's own
            err_n, err_p = np.abs(net_h[e] - ref_net), np.abs(pf_h[e] - ref_pf)
            bound_n, bound_p = np.concatenate([c * EPS * mag[:, :3], (c + 3) * EPS * mag[:, 3:]], 1), c * EPS * pmag
            print("contact report, reducer: env %d: count %d, bodies in contact %d, sensor / filter pairs in contact %d, largest net entry %.3e, "
                  "largest difference %.2e net, %.2e pair" % (e, c, int((mag[:, 0] > 0).sum()), int((pmag.sum(-1) > 0).sum()), np.abs(ref_net).max(),
                                                              err_n.max(), err_p.max()))
            assert (err_n <= bound_n).all(), (e, float(err_n.max()))
            assert (err_p <= bound_p).all(), (e, float(err_p.max()))
            quiet = mag.sum(1) == 0
            assert quiet.sum() >= NB - NF - NL and (net_h[e][quiet].view(np.uint32) == 0).all()       # bodies without contacts: +0 exactly
            assert (pf_h[e][pmag.sum(-1) == 0].view(np.uint32) == 0).all()
            outs.append((int((pmag.sum(-1) > 0).sum()), int((~quiet).sum())))
        assert outs[1] == (0, 0) and outs[0][1] > NF // 2 and outs[0][0] >= 1 and outs[2][0] >= 1, outs
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 7. full size (GPU only)
def case_full_size(backend, n=1024, steps=8):
    """the default scene at N = 1 024, 8 sdx_steps with the report armed against a second simulator without it"""
    make, dev = backend
    a, b = make(n, seed=22), make(n, seed=22)
    try:
        rep = a.contact_report()
        g = torch.Generator().manual_seed(4)
        for _ in range(steps):
            act = dev(torch.rand(n, ND, generator=g) * 2 - 1)
            a.step(act)
            b.step(act)
        for k in ("ROOT", "DOF"):
            assert torch.equal(a.tensor(k).view(torch.int32), b.tensor(k).view(torch.int32)), k
        assert torch.equal(a.CONTACT_STATS, b.CONTACT_STATS)
        nc = a.NCONTACTS
        assert torch.equal(rep.count, nc.clamp(max=M)) and torch.equal(nc, b.NCONTACTS)
        print("contact report, full size: N %d, contacts per env %d .. %d, CONTACT_STATS %s" % (n, int(nc.min()), int(nc.max()), host(a.CONTACT_STATS).tolist()))
        assert int(nc.max()) > 0
    finally:
        a.close()
        b.close()
