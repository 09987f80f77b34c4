"""TEST INFRASTRUCTURE ONLY: numpy restatement of the view camera (seqdex_amd/csrc/sdx_camera.hip k_view_render, include/seqdex.h
sdx_render_view): the same boxes in the same order, the same pinhole model, the brute-force slab loop the kernel's result is defined by,
in fp32 and operation by operation (the kernel's view section is compiled without FMA contraction), so that coplanar faces tie the same
way.  Returns depth, label, rgb and the entering axis per pixel.  PARITY UNPINNED against Isaac Gym's renderer."""
import numpy as np

from oracle.camera_oracle import quat_apply, quat_mul, scene_boxes

F = np.float32
BOUNDS, COLLISION = 0, 1
NFREE, NBRICK = 72, 132

# class colours: background, target brick, brick types 0..7, fixed bricks, arm links, hand links, table, bin, floor, plate
COLORS = np.array([[24, 26, 32], [255, 48, 48],
                   [66, 135, 245], [60, 180, 75], [255, 225, 25], [245, 130, 48], [145, 30, 180], [70, 240, 240], [240, 50, 230], [170, 110, 40],
                   [128, 128, 140], [200, 200, 210], [250, 190, 150], [120, 90, 60], [90, 110, 130], [150, 150, 120], [0, 128, 128]], F)
C_BACKGROUND, C_TARGET, C_TYPE0, C_FIXED, C_ARM, C_HAND, C_TABLE, C_BIN, C_FLOOR, C_PLATE = 0, 1, 2, 10, 11, 12, 13, 14, 15, 16


def seg_brick(env):
    b = env & 7
    return 0 if b in (3, 4, 7) else b


def _static_class(slot):
    return C_TABLE if slot == 0 else (C_BIN if slot < 6 else (C_FLOOR if slot == 6 else C_PLATE))


def _qrot(q, v):
    """quat_apply written out in the kernel's operation order (fp32)"""
    q, v = np.asarray(q, F), np.asarray(v, F)
    u = q[:3]
    cr = lambda a, b: np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)
    t = cr(u, v) * F(2.0)
    return ((v + t * q[3]) + cr(u, t)).astype(F)


def _qmul(a, b):
    x1, y1, z1, w1 = [F(x) for x in a]
    x2, y2, z2, w2 = [F(x) for x in b]
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], F)


def boxes(desc, root_env, rb_env, env, geometry):
    """(centres [B,3], quats [B,4], halves [B,3], labels [B], classes [B]) of env `env` (its index decides the target brick and, for
    InsertSim, the base plate), in the kernel's box order"""
    bt = np.array(list(desc.brick_type))
    segb = seg_brick(env)
    ns, nr = desc.n_static, desc.n_rbox
    c, q, h, lab, cls = [], [], [], [], []
    ident = np.array([0, 0, 0, 1], F)

    def brick_class(i):
        return C_TARGET if i == segb else (C_TYPE0 + int(bt[i]) if i < NFREE else C_FIXED)

    for i in range(NBRICK):
        r = root_env[9 + i].astype(F)
        t = int(bt[i])
        if geometry == COLLISION and i < NFREE:
            if desc.seg_hollow and i == segb:
                subs = [(list(desc.hollow_sub_center[t][k]), list(desc.hollow_sub_half[t][k])) for k in range(desc.hollow_nsub[t])]
            else:
                subs = [(list(desc.brick_sub_center[t][k]), list(desc.brick_sub_half[t][k])) for k in range(desc.brick_nsub[t])]
        else:
            subs = [(list(desc.brick_center[t]), list(desc.brick_half[t]))]
        for off, hh in subs:
            c.append(r[0:3] + _qrot(r[3:7], np.array(off, F)))
            q.append(r[3:7]); h.append(np.array(hh, F)); lab.append(i + 1); cls.append(brick_class(i))
    for s in range(ns):
        if geometry == COLLISION:
            row = desc.static_var_row[env % 3] if s == desc.static_var_slot else s
            first, n = desc.static_sub_first[row], desc.static_sub_n[row]
            subs = [(list(desc.static_sub_center[k]), list(desc.static_sub_half[k])) for k in range(first, first + n)]
        else:
            subs = [(list(desc.static_center[s]), list(desc.static_half[s]))]
        for cc, hh in subs:
            c.append(np.array(cc, F)); q.append(ident); h.append(np.array(hh, F)); lab.append(-100 - s); cls.append(_static_class(s))
    for k in range(nr):
        l = int(desc.rbox_link[k])
        ql = rb_env[l, 3:7].astype(F)
        c.append(rb_env[l, 0:3].astype(F) + _qrot(ql, np.array(list(desc.rbox_center[k]), F)))
        q.append(_qmul(ql, np.array(list(desc.rbox_quat[k]), F)))
        h.append(np.array(list(desc.rbox_half[k]), F)); lab.append(-1 - l); cls.append(C_ARM if l < desc.hand_base_body else C_HAND)
    return (np.array(c, F).reshape(-1, 3), np.array(q, F).reshape(-1, 4), np.array(h, F).reshape(-1, 3), np.array(lab, np.int64),
            np.array(cls, np.int64))


def camera_basis(cam, rb_env):
    """(origin, f, r, u) in the env frame, fp32, the kernel's operations"""
    pos, tgt, up = np.array(cam.pos, F), np.array(cam.target, F), np.array(cam.up, F)
    if cam.attach_body >= 0:
        lp, lq = rb_env[cam.attach_body, 0:3].astype(F), rb_env[cam.attach_body, 3:7].astype(F)
        pos, tgt, up = lp + _qrot(lq, pos), lp + _qrot(lq, tgt), _qrot(lq, up)
    cr = lambda a, b: np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)
    dot = lambda a, b: F(F(a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])
    f = tgt - pos
    f = f * (F(1.0) / np.sqrt(dot(f, f)))
    r = cr(f, up)
    r = r * (F(1.0) / np.sqrt(dot(r, r)))
    return pos.astype(F), f.astype(F), r.astype(F), cr(r, f)


def render_boxes(c, q, h, lab, cls, origin, f, r, u, hfov_deg, W, H):
    """the brute-force loop over boxes in order: depth f32 [H,W] (+inf: nothing), label i16, rgb u8 [H,W,3], entering axis i8 (-1: none)"""
    th = F(np.tan(F(F(0.5) * F(hfov_deg)) * F(0.017453292519943295)))
    tv = F(F(th * F(H)) / F(W))
    cols, rows = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    px = ((F(2.0) * (cols + F(0.5)) / F(W) - F(1.0)) * th).astype(F)
    py = ((F(1.0) - F(2.0) * (rows + F(0.5)) / F(H)) * tv).astype(F)
    d = [(f[a] + r[a] * px) + u[a] * py for a in range(3)]                      # [3][H,W]
    best = np.full((H, W), 3.0e38, F)
    best_i = np.full((H, W), -1, np.int64)
    best_ax = np.full((H, W), -1, np.int8)
    best_nd = np.full((H, W), -1.0, F)
    for b in range(c.shape[0]):
        M = np.stack([_qrot(q[b], e) for e in np.eye(3, dtype=F)])              # rows = box axes in world coordinates
        dd = origin - c[b]
        o = [F(F(M[a, 0] * dd[0] + M[a, 1] * dd[1]) + M[a, 2] * dd[2]) for a in range(3)]
        if all(abs(o[a]) < h[b, a] for a in range(3)):                          # the box strictly contains the ray origin: skipped
            continue
        tmin = np.zeros((H, W), F)
        tmax = np.full((H, W), 3.0e38, F)
        nd = np.full((H, W), -1.0, F)
        ax = np.full((H, W), -1, np.int8)
        hit = np.ones((H, W), bool)
        for a in range(3):
            da = ((M[a, 0] * d[0] + M[a, 1] * d[1]) + M[a, 2] * d[2]).astype(F)
            par = np.abs(da) < F(1e-12)
            if abs(o[a]) > h[b, a]:
                hit &= ~par
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                inv = (F(1.0) / np.where(par, F(1.0), da)).astype(F)
                t0, t1 = ((-h[b, a] - o[a]) * inv).astype(F), ((h[b, a] - o[a]) * inv).astype(F)
            lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
            enter = ~par & (lo > tmin)
            tmin = np.where(enter, lo, tmin)
            nd = np.where(enter, np.abs(da), nd)
            ax = np.where(enter, np.int8(a), ax)
            tmax = np.where(par, tmax, np.minimum(tmax, hi))
        hit &= (tmin <= tmax) & (tmin < best)
        best = np.where(hit, tmin, best)
        best_i = np.where(hit, b, best_i)
        best_ax = np.where(hit, ax, best_ax)
        best_nd = np.where(hit, nd, best_nd)
    got = best_i >= 0
    depth = np.where(got, best, F(np.inf)).astype(F)
    label = np.where(got, lab[np.maximum(best_i, 0)], 0).astype(np.int16)
    klass = np.where(got, cls[np.maximum(best_i, 0)], C_BACKGROUND)
    dn = np.sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(F)).astype(F)
    shade = np.where(got & (best_nd >= 0), F(0.35) + F(0.65) * (best_nd / dn).astype(F), F(1.0)).astype(F)
    rgb = np.floor(COLORS[klass] * shade[..., None] + F(0.5)).astype(np.uint8)
    return depth, label, rgb, np.where(got, best_ax, -1).astype(np.int8)


def render(desc, root_env, rb_env, env, cam, W, H, geometry=COLLISION):
    """cam: anything with pos, target, up, attach_body, hfov_deg (seqdex_amd.view.ViewCamera)"""
    c, q, h, lab, cls = boxes(desc, root_env, rb_env, env, geometry)
    origin, f, r, u = camera_basis(cam, rb_env)
    return render_boxes(c, q, h, lab, cls, origin, f, r, u, cam.hfov_deg, W, H)


def failing_share(got, want):
    """the share rule: got = (depth, label, rgb) of the kernel, want = (depth, label, rgb, axis) of this helper.  A pixel fails when its
    label differs, its depth differs by more than 1e-5 m (inf == inf), or - label equal - a colour channel differs by more than 1.  (The
    kernel does not output the entering axis; with the label and the depth equal it entered through the helper's face unless two faces of
    the box are hit at once, an edge pixel, which then counts against the kernel.)  depth / rgb of `got` may be None (output not asked for)."""
    depth, label, rgb = got
    wd, wl, wrgb, _ = want
    bad = label != wl if label is not None else np.zeros(wl.shape, bool)
    if depth is not None:
        both_inf = np.isinf(depth) & np.isinf(wd)
        with np.errstate(invalid="ignore"):
            bad = bad | (~both_inf & ~(np.abs(depth - wd) <= 1e-5))
    if rgb is not None:
        bad = bad | (~bad & (np.abs(rgb.astype(np.int32) - wrgb.astype(np.int32)).max(-1) > 1))
    return float(bad.mean())


__all__ = ["render", "boxes", "camera_basis", "render_boxes", "failing_share", "seg_brick", "COLORS", "BOUNDS", "COLLISION",
           "quat_apply", "quat_mul", "scene_boxes"]


def scattered_bricks(n, seed=0):
    """[n, 72, 7] poses of the free bricks scattered over the bin with random orientations: the scene of
    tests/test_gpu_search_parity.py::test_segmentation_camera_matches_numpy_ray_caster (same generator, same draws)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    out = np.zeros((n, 72, 7), np.float32)
    for e in range(n):
        out[e, :, 0] = (0.05 + 0.4 * torch.rand(72, generator=g)).numpy()
        out[e, :, 1] = (0.02 + 0.34 * torch.rand(72, generator=g)).numpy()
        out[e, :, 2] = (0.63 + 0.12 * torch.rand(72, generator=g)).numpy()
        q = torch.randn(72, 4, generator=g)
        out[e, :, 3:7] = (q / q.norm(dim=1, keepdim=True)).numpy()
    return out
