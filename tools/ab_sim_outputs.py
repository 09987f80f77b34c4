"""Does the simulator of two trees (or two builds of the library) compute the same?  One seeded run of all four task kinds, every tensor
of _abi.T dumped; a second mode compares two dumps bit for bit.

    python tools/ab_sim_outputs.py run --tree TREE --backend emu --envs 16 --out DIR     the kernel SOURCES of TREE on tests/hipemu (CPU)
    SDX_LIB_PATH=.../libseqdex_hip.so python tools/ab_sim_outputs.py run --backend gpu --envs 64 --out DIR      a compiled library
    python tools/ab_sim_outputs.py diff DIR_A DIR_B [--out report.txt] [--title "parent vs result"]             exit 1 on a difference

Per task kind: the constructor arguments of the fixtures of tests/test_hipemu_task_parity.py with max_episode_length = 5, T-value weights
that accept every state, seeded uniform actions.  Phase 1 (randomization off): 7 steps (the reset event of the first step and the one
after the time-out), a masked reset_idx with both outcomes of the accept rules' inputs, compute_observations.  Phase 2: randomization on
with every attribute sampled, observation and action noise on, 3 steps (one with a due refresh), save_all / step / restore_all / step, one
clone.  Every tensor of _abi.T is dumped after each phase, the rings through ring_rows (their sorted keys as *_keys)."""
import argparse
import os
import sys

import numpy as np

KINDS = [dict(), dict(task_kind=1), dict(task_kind=2), dict(task_kind=3, act_moving_average=0.6, target_euler=[0.0, 3.14, 1.57])]
RINGS = {"HARVEST_HAND": ("HARVEST_KEYS", "HARVEST_COUNT"), "HARVEST_OBJ": ("HARVEST_KEYS", "HARVEST_COUNT"),
         "PILE_HARVEST": ("PILE_HARVEST_KEYS", "PILE_HARVEST_COUNT"), "TV_SUCCESS": ("TV_KEYS", "TV_COUNT"), "TV_FAILURE": ("TV_KEYS", "TV_COUNT")}
KEY_TENSORS = {"HARVEST_KEYS", "PILE_HARVEST_KEYS", "TV_KEYS"}      # dumped with their rings, in sorted order


def backend(name, tree):
    import torch
    if name == "emu":
        sys.path[:0] = [tree, os.path.join(tree, "tests")]
        import tests.hipemu as H
        from tests.hipemu.sim import EmuSim
        assert os.path.samefile(H.ROOT, tree), "tests.hipemu was imported from %s, not from %s" % (H.ROOT, tree)
        return (lambda n, **kw: EmuSim(n, **kw)), (lambda t: t), (lambda: None)
    sys.path.insert(0, tree)
    from seqdex_amd.sim import SdxSim
    return (lambda n, **kw: SdxSim(n, device="cuda:0", **kw)), (lambda t: t.cuda()), torch.cuda.synchronize


def accept_all(n_params):
    w = np.zeros(n_params, np.float32)      # every layer's output is its bias: the head ends in (ELU(-10), 10), sigmoid(.)[1] = 1
    w[-2:] = (-10.0, 10.0)
    return w


def ring(s, name):
    """(rows, keys, count) of the parts of one ring: the T-value rings have one (success / failure), the harvest rings one per brick type"""
    keys, count = s.tensor(RINGS[name][0]), s.tensor(RINGS[name][1])
    rows = s.tensor(name)
    if name.startswith("TV_"):
        g = 0 if name == "TV_SUCCESS" else 1
        return [(rows, keys[g], int(count[g]))]
    return [(rows[t], keys[t], int(count[t])) for t in range(8)]


def dump(s, sync, out, tag):
    import torch
    from seqdex_amd import _abi
    sync()
    for name in _abi.T:
        if name in KEY_TENSORS:
            continue
        if name in RINGS:
            parts, kparts = [], []
            for rows, keys, count in ring(s, name):
                k = min(count, rows.shape[0])
                parts.append(s.ring_rows(rows, keys, count).flatten(1))
                kparts.append(torch.sort(keys[:k])[0])
            np.save(os.path.join(out, "%s_%s.npy" % (tag, name)), torch.cat(parts).cpu().numpy())
            np.save(os.path.join(out, "%s_%s_keys.npy" % (tag, name)), torch.cat(kparts).cpu().numpy())
        else:
            np.save(os.path.join(out, "%s_%s.npy" % (tag, name)), s.tensor(name).cpu().numpy())
    assert not getattr(s, "ring_wrapped", False)


def full_desc(frequency):
    """every attribute of sdx_dr_desc sampled: all three distributions, both operations, a schedule and buckets among them"""
    from seqdex_amd import domain_randomization as dr
    d = dr.identity_desc(frequency)
    spec = {"gravity": (1, 1, (0.0, 0.4), 0, 0, 0), "dof_stiffness": (3, 2, (0.75, 1.5), 0, 0, 0), "dof_damping": (3, 2, (0.3, 3.0), 1, 3000, 0),
            "dof_lower": (1, 1, (0.0, 0.01), 0, 0, 0), "dof_upper": (1, 1, (0.0, 0.01), 2, 1, 0), "link_mass": (2, 2, (0.5, 1.5), 0, 0, 0),
            "link_friction": (2, 2, (0.7, 1.3), 0, 0, 250), "brick_mass": (2, 2, (0.5, 1.5), 1, 3000, 0), "brick_friction": (2, 1, (-0.1, 0.1), 0, 0, 4)}
    for f, (dist, op, rng, sched, steps, buckets) in spec.items():
        a = getattr(d, f)
        a.distribution, a.operation, a.schedule, a.schedule_steps, a.num_buckets = dist, op, sched, steps, buckets
        a.range[0], a.range[1] = rng
    return d


def noise_attr(distribution, operation, rng, corr):
    from seqdex_amd import _abi
    a = _abi.NoiseAttr()
    a.distribution, a.operation, a.schedule, a.schedule_steps = distribution, operation, 1, 3000
    a.range[0], a.range[1] = rng
    a.range_correlated[0], a.range_correlated[1] = corr
    return a


def run_kind(kind, make, dev, sync, n, out):
    import torch
    from seqdex_amd import _abi
    s = make(n, seed=22, max_episode_length=5.0, **KINDS[kind])
    try:
        s.set_tvalue_weights(accept_all(_abi.TV_PARAMS))
        if kind == 3:
            s.set_retri_tvalue_weights(accept_all(_abi.RETRI_TV_PARAMS))
        g = torch.Generator().manual_seed(1000 + kind)
        acts = [dev((torch.rand(n, 23, generator=g) * 2.4 - 1.2).contiguous()) for _ in range(16)]     # some outside the +-1 clamp
        # ---- phase 1: randomization off
        env = torch.arange(n)
        if kind == 2:                                  # InsertSim resets from GraspSim's terminal states: five per type group, filled by hand
            s.HARVEST_HAND[:, :5] = s.DOF.reshape(n, 23, 2)[:5].clone()
            s.HARVEST_OBJ[:, :5] = s.ROOT.reshape(n, 142, 13)[:5, 9:17].transpose(0, 1).clone()
            s.HARVEST_KEYS[:, :5] = dev(torch.arange(5))
            s.HARVEST_COUNT[:] = 5
        for i in range(7):
            s.step(acts[i])
        sync()
        # the accept rules' inputs by hand, so that both outcomes occur among the masked envs: an accepting T-value on the odd envs, closed
        # fingers everywhere, and (GraspSim's rule: the target brick over the base plate, y < 0) the bricks of envs 1, 2 mod 4 moved there
        odd = dev((env % 2).to(torch.float32))
        s.TVALUE[:] = 0.9 * odd + 0.05
        s.SUCCESSES[:] = odd
        s.FINGER_DIST[:] = 0.1
        s.ROOT.reshape(n, 142, 13)[:, 9:141, 1] -= dev((((env % 4) == 1) | ((env % 4) == 2)).to(torch.float32))[:, None]
        mask = dev(((torch.arange(n) % 3) != 1).to(torch.uint8))
        s.reset_idx(mask, dev(torch.zeros(n, dtype=torch.int32)))      # the pile choice must lie in [0, K): one saved pile per type here
        s.compute_observations()
        dump(s, sync, out, "k%d_p1" % kind)
        # ---- phase 2: randomization with every attribute sampled, both noise blocks, snapshots
        s.DR_FRAME[0] = 1500
        s.set_randomization(full_desc(2))
        s.set_noise(observations=noise_attr(1, 1, (0.001, 0.002), (-0.0005, 0.001)), actions=noise_attr(2, 2, (0.95, 1.04), (0.99, 1.02)))
        for i in range(3):
            if i == 1:                                 # a due refresh: every env resets with randomize_buf past the frequency
                s.DR_FRAME[0] = 1510
                s.RESET[:] = 1
                s.RANDOMIZE[:] = 5
            s.step(acts[7 + i])
        st = s.snapshot()
        st.save()
        s.step(acts[10])
        st.restore()
        s.step(acts[11])
        # clone env e -> e + 24 (the same class for every task: 24 = lcm(8, 3)) where both exist, else e -> e + 8 for the tasks that allow it
        far = 24 if n > 24 else 8
        pairs = [(e, e + far) for e in range(min(4, n - far)) if s.env_class(e) == s.env_class(e + far)]
        if pairs:
            s.clone_envs([a for a, _ in pairs], [b for _, b in pairs])
        s.step(acts[12])
        sync()
        np.save(os.path.join(out, "k%d_p2_state_stats.npy" % kind), np.asarray(s.state_stats(), np.int32))
        np.save(os.path.join(out, "k%d_p2_cloned_pairs.npy" % kind), np.asarray(pairs, np.int32).reshape(-1, 2))
        dump(s, sync, out, "k%d_p2" % kind)
        st.close()
        sync()
        return "kind %d  TV_COUNT %s  HARVEST_COUNT %s  PILE_HARVEST_COUNT %s  DR_FRAME %s  clones %d" % (
            kind, s.TV_COUNT.cpu().tolist(), s.HARVEST_COUNT.cpu().tolist(), s.PILE_HARVEST_COUNT.cpu().tolist(), s.DR_FRAME.cpu().tolist(), len(pairs))
    finally:
        s.close()


def cmd_run(a):
    tree = os.path.abspath(a.tree)
    make, dev, sync = backend(a.backend, tree)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "exercised.txt"), "w") as fh:
        for kind in range(4):
            line = run_kind(kind, make, dev, sync, a.envs, a.out)
            print(line, flush=True)
            fh.write(line + "\n")
    return 0


def cmd_diff(a):
    names = sorted(f for f in set(os.listdir(a.a)) | set(os.listdir(a.b)) if f.endswith(".npy"))
    lines, bad, worst = ["== " + a.title], 0, 0.0
    for side in (a.a, a.b):
        p = os.path.join(side, "exercised.txt")
        if os.path.exists(p):
            lines += ["# what the run exercised, %s:" % os.path.basename(os.path.normpath(side))] +["#   " + l.rstrip() for l in open(p)]
    for f in names:
        pa, pb = os.path.join(a.a, f), os.path.join(a.b, f)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            lines.append("  %-34s only in %s" % (f[:-4], a.a if os.path.exists(pa) else a.b))
            bad += 1
            continue
        x, y = np.load(pa), np.load(pb)
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        d = float(np.max(np.abs(x.astype(np.float64) - y.astype(np.float64)))) if x.shape == y.shape and x.size else (0.0 if same else float("inf"))
        d = d if d == d else float("inf")
        worst = max(worst, d)
        bad += not same
        lines.append("  %-34s %-18s max|diff| %.3e %s" % (f[:-4], x.shape, d, "bit-identical" if same else "DIFFERS"))
    lines.append("%s: %d arrays, %d not bit-identical, worst %.3e" % (a.title, len(names), bad, worst))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text)
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to import seqdex_amd (and tests.hipemu) from")
    r.add_argument("--backend", choices=("emu", "gpu"), required=True)
    r.add_argument("--envs", type=int, default=16)
    r.add_argument("--out", required=True)
    d = sub.add_parser("diff")
    d.add_argument("a")
    d.add_argument("b")
    d.add_argument("--out", default="", help="append the report to this file")
    d.add_argument("--title", default="A vs B")
    a = ap.parse_args()
    return cmd_run(a) if a.cmd == "run" else cmd_diff(a)


if __name__ == "__main__":
    sys.exit(main())
