"""The scripted stand-in for a trained BlockAssemblyGraspSim policy and the two lift statistics (can the hand lift a brick? what does a
trained policy physically do?).  The chain benchmarks, the bi-optimisation loop's stand-in legs and tests/test_gpu_scripted_lift.py use them."""
import os

import torch

from ..stage import make_task

# closure, pinch steps, rise per step, pinch height, pinch offset x / y.  Round 5 (profiles/r5_scripted_lift_scan.txt): the pinch height decides -
# 0.195 above the brick's origin (rounds 3-4) the fingertips close over the studs and 18 % of 1 024 envs hold the brick 5 cm up; at 0.155 they
# close on the brick's body: 54 %
SG_DEFAULTS = [0.9, 8.0, 0.05, 0.155, 0.125, 0.02]


def scripted_grasp_controller(task, step):
    """STAND-IN for a trained BlockAssemblyGraspSim policy (the reference's released checkpoint is from epoch 19 000, README.md:90; nothing of
    that length can be trained inside a test): a hand-written reach - descend - pinch sequence on the task's own action interface
    (GS:1586-1609: a[0:3] x 0.64 = hand-base displacement for the IK, a[3:6] x 0.2 = wrist orientation error, a[7:23] = finger targets scaled
    to the joint limits): hand base above the target brick with the wrist held at the prepare pose's orientation, descend, pinch when
    arrived (at the latest at step 58); once the pinch is complete the hand stops following the brick (a gripped brick moves with the hand)
    and raises it a little.  After step 75 the task itself lifts the hand and carries it to the insertion side with the fingers frozen
    (GS:1600-1609).  SDX_SG_PARAMS="closure,steps,rise,height,x,y" overrides the pinch's end closure / duration, the rise per step, the height
    of the hand base above the brick at the pinch and the pinch point's offset from the hand base (tools/lift_diag.py).  Used by tools/bench_config3.py, tools/bench_config5.py and tests/test_gpu_chain.py so that the grasp stage
    harvests REAL terminal states of this engine; success is far below a trained policy's.  One kernel launch per env step
    (csrc/sdx_task.hip::k_scripted_grasp; round 3 computed the same in ~40 torch operations inside the timed loop)."""
    import ctypes as C
    s = task.sim
    if not hasattr(task, "_sg_close"):
        # per env: the progress values at which the fingers started to close / the hand stopped following the brick; then the parameters
        par = SG_DEFAULTS[:]
        for i, x in enumerate(os.environ.get("SDX_SG_PARAMS", "").split(",")):
            if x.strip():
                par[i] = float(x)
        task._sg_close = torch.cat([torch.full((2 * task.num_envs,), 1e9), torch.tensor(par + [0.0, 0.0])]).to(task.device).contiguous()
        task._sg_act = torch.zeros(task.num_envs, 23, device=task.device)
        s.lib.sdxk_scripted_grasp_actions.restype = C.c_int
        s.lib.sdxk_scripted_grasp_actions.argtypes = [C.c_void_p] * 4
    rc = s.lib.sdxk_scripted_grasp_actions(s.h, C.c_void_p(task._sg_close.data_ptr()), C.c_void_p(task._sg_act.data_ptr()),
                                           C.c_void_p(torch.cuda.current_stream(task.device).cuda_stream))
    if rc != 0:
        raise RuntimeError("sdxk_scripted_grasp_actions failed (%d)" % rc)
    return task._sg_act



def scripted_lift_statistics(num_envs=1024, seed=22, piles_per_type=16):
    """can the hand lift a brick?  One episode of BlockAssemblyGraspSim under the scripted controller; per env the
    largest height the target brick reached above its initial one WHILE finger_dist < 0.5 (GS:1164-1165; the reward's own "in the hand"
    threshold, GS:1725), first episode only.  Returns a dict with the fraction of envs that held it >= 5 cm up."""
    task = make_task("BlockAssemblyGraspSim", num_envs, seed, piles_per_type=piles_per_type)
    try:
        s, n, dev = task.sim, num_envs, task.device
        seg = torch.as_tensor([s.scene.seg_index(i) for i in range(n)], device=dev)
        ar = torch.arange(n, device=dev)
        task.step(torch.zeros(n, 23, device=dev))                              # the reset step
        z0 = s.INIT_POS[:, 2].clone()
        held = torch.zeros(n, device=dev)
        first = torch.ones(n, dtype=torch.bool, device=dev)
        for step in range(1, int(task.max_episode_length)):
            task.step(scripted_grasp_controller(task, step))
            first &= s.PROGRESS > 1                                            # a reset env is out of its first episode
            dz = s.ROOT.view(n, 142, 13)[ar, seg, 2] - z0
            held = torch.where(first & (s.FINGER_DIST < 0.5), torch.maximum(held, dz), held)
        torch.cuda.synchronize()
        ok = held > 0.05
        return {"n": n, "held_5cm_frac": float(ok.float().mean()), "held_2cm_frac": float((held > 0.02).float().mean()),
                "held_max_m": float(held.max()), "per_type_held_5cm": [int(ok[ar % 8 == g].sum()) for g in range(8)],
                "contact_stats": s.CONTACT_STATS.cpu().tolist()}
    finally:
        task.sim.close()


def policy_lift_statistics(task, agent, steps=304):
    """what a TRAINED grasp policy physically does (round 5, the check behind the training curves): `steps` deterministic env steps (two
    episodes) of `agent` on `task`; per env the largest height of the target brick above its initial one while finger_dist < 0.5, whether at
    least two fingertip links (thumb among them) carried a net contact force > 0.5 N at that moment (held BY contacts, not by a brick lying
    on the hand), and the brick's speed relative to the hand base then.  Sampled after every env step of the horizon-sized chunks."""
    s, n, dev = task.sim, task.num_envs, task.device
    seg = torch.as_tensor([s.scene.seg_index(i) for i in range(n)], device=dev)
    ar = torch.arange(n, device=dev)
    tips = list(s.scene.fingertip_bodies)
    held = torch.zeros(n, device=dev)
    grip = torch.zeros(n, dtype=torch.bool, device=dev)
    rel = torch.zeros(n, device=dev)
    eps = torch.zeros(n, agent.ppo.cfg.act_dim, device=agent.ppo.device)
    if agent.obs is None:
        agent.obs = agent.env_reset()
        agent.dones = agent.vec_env.task.reset_buf
    for k in range(steps):
        a = agent.ppo.act(k % agent.horizon_length, agent.obs["obs"], agent.obs["states"], agent.dones, eps)
        agent.obs, rew, agent.dones, _ = agent.vec_env.step(a)
        b = s.ROOT.view(n, 142, 13)[ar, seg]
        dz = b[:, 2] - s.INIT_POS[:, 2]
        cf = s.CONTACT.view(n, 165, 3)[:, tips].norm(dim=-1)
        g2 = (cf[:, 3] > 0.5) & ((cf[:, :3] > 0.5).sum(1) >= 1)
        better = (s.FINGER_DIST < 0.5) & (dz > held) & (s.PROGRESS > 1)
        held = torch.where(better, dz, held)
        grip = torch.where(better, g2, grip)
        rel = torch.where(better, (b[:, 7:10] - s.RB[:, s.scene.hand_base_body, 7:10]).norm(dim=-1), rel)
    torch.cuda.synchronize()
    ok = held > 0.05
    return {"steps": steps, "held_5cm_frac": float(ok.float().mean()), "held_15cm_frac": float((held > 0.15).float().mean()), "held_max_m": float(held.max()),
            "of_those_gripped_by_thumb_and_a_finger": float((ok & grip).float().sum() / ok.float().sum().clamp(min=1)),
            "brick_speed_relative_to_hand_at_the_top_mean_m_s": float(rel[ok].mean()) if bool(ok.any()) else None,
            "per_type_held_5cm": [int(ok[ar % 8 == g].sum()) for g in range(8)]}
