"""Training recipes of the chain on this engine's own policies, and the chains that compose them (rounds 5-6): an insert policy and the
transition value fitted to its outcomes (the backward leg of the reference's scripts/bi_optimization.py:120-121 in small), a grasp and an
Orient policy trained under that value, then scripts/evaluation.py's chain played on the result.  Every stage is built by
seqdex_amd.stage.make_stage; the recipes differ in their task arguments, in whose weights gate the harvest and in what they report.
tools/chain_learned.py and tools/chain_closed.py report the chains, tests/test_gpu_chain.py pins the closed one."""
import os
import tempfile
import time

import numpy as np
import torch

from ..stage import make_stage
from ..tvalue_trainer import LAYERS, TValue_Trainer, flat_from_state_dict, open_gate_weights
from .evaluation import block_assembly_chain, main_rlgames
from .scripted_grasp import policy_lift_statistics

GRASP_TRAIN_MINIBATCH = 2048     # the minibatch size GraspSim LEARNS with on this engine (profiles/r5_grasp_train_curve_*.txt); the YAML ships 4


def _train(agent, epochs):
    """`epochs` training epochs -> (wall seconds, game reward after the first 100 epochs - or after the last one of fewer)"""
    t0, early = time.time(), None
    for ep in range(epochs):
        agent.train_epoch()
        if ep == min(99, epochs - 1):
            early = float(agent.game_rewards.get_mean()[0])
    torch.cuda.synchronize()
    return time.time() - t0, early


def _save(agent, save_to):
    """-> the path of the checkpoint written (A2CAgent.save appends .pth), "" without save_to"""
    if not save_to:
        return ""
    agent.save(save_to)
    return save_to + ".pth"


def train_grasp_policy(n, epochs, seed=22, save_to=None, minibatch=GRASP_TRAIN_MINIBATCH, tvalue_state=None, initial_piles=None, piles_per_type=16, lift_statistics=False,
                       restore=""):
    """A BlockAssemblyGraspSim policy of THIS engine (round 5; the reference's is its released 19 000-epoch checkpoint, README.md:90):
    `epochs` epochs at n envs, horizon 8, 5 mini-epochs, adaptive learning rate as shipped - but minibatches of 2 048 rows instead of the
    shipped 4, with which the shipped schedule does not leave reward 2 (profiles/r5_grasp_train_curve_shipped_minibatch4.txt); episode reward
    ~ 2 000 after 1 500 epochs = 30 s (the reference's checkpoint name says 1 531).  tvalue_state: the transition value that gates the
    harvest of grasp terminal states (GS:1404-1417; None: the gate is opened - what a forward leg of the bi-optimisation loop does before
    any T-value exists).  restore: a grasp checkpoint to go on from (a later round of the bi-optimisation loop fine-tunes the policy under the
    refitted value).  Returns (checkpoint path or "", the task (caller closes task.sim; its rings hold the harvested states), statistics)."""
    task, env, agent = make_stage("BlockAssemblyGraspSim", n, seed, task_kwargs={"initial_piles": initial_piles, "piles_per_type": piles_per_type},
                                  minibatch_size=minibatch, restore=restore)
    task.sim.set_tvalue_weights(open_gate_weights() if tvalue_state is None else tvalue_state)
    wall, _ = _train(agent, epochs)
    st = {"epochs": epochs, "restored_from": restore or None, "minibatch_size": minibatch, "wall_s": wall, "game_reward": float(agent.game_rewards.get_mean()[0]),
          "game_length": float(agent.game_lengths.get_mean()[0]), "grasp_states_harvested_per_type": task.sim.HARVEST_COUNT.cpu().tolist(),
          "tvalue_gate": "open" if tvalue_state is None else "given", "contact_stats": task.sim.CONTACT_STATS.cpu().tolist()}
    if lift_statistics:
        st["deterministic_play"] = policy_lift_statistics(task, agent)
    path = _save(agent, save_to)
    agent.ppo.close()
    return path, task, st


def prepare_tvalue_and_insert_policy(n, epochs, fit_iters=10000, seed=22, save_to=None, grasp_states=None, restore="", synthetic_fallback=False, fit=True):
    """stage 0 of the chain (untimed; the backward pass of scripts/bi_optimization.py:120-121 in small): BlockAssemblyInsertSim trains
    `epochs` epochs with its shipped schedule from synthetic grasp states (or, grasp_states given, from grasp terminal states a grasp
    policy harvested), its episode outcomes fill the T-value rings, GraspInsertTValue
    is fitted to them -> the transition value that gates the harvests of the chain, and the insert policy of its last stage.
    Deterministic run to run: torch's global generator is seeded like the launcher does (it feeds VecTask.reset()'s noise step), training
    is (fixed-order reductions, counter-based noise) and the fit reads the outcome rings in serial (step, env) order (SdxSim.ring_rows),
    not in the order the slots were claimed in.
    restore: an insert checkpoint to go on from (the forward leg of a later bi-optimisation round: the policy that learned on synthetic
    states is fine-tuned on the states a grasp policy harvested); synthetic_fallback: brick-type groups without a harvested state start from
    synthetic states (named in the statistics); fit=False: no transition-value fit (returns None for it).
    Returns (flat T-value weights or None, insert checkpoint path or "", statistics)."""
    task, env, agent = make_stage("BlockAssemblyInsertSim", n, seed, task_kwargs={"grasp_states": grasp_states, "synthetic_fallback": synthetic_fallback},
                                  restore=restore)
    wall, _ = _train(agent, epochs)
    sb = task.extras["success_buf"].float()
    real = torch.tensor([(e % 8) not in task.synthetic_groups for e in range(n)], device=sb.device)
    st = {"epochs": epochs, "wall_s": wall, "game_reward": float(agent.game_rewards.get_mean()[0]), "grasp_states": task.grasp_states_source,
          "restored_from": restore or None, "outcomes_logged(success, failure)": task.sim.TV_COUNT.cpu().tolist(),
          "insert_success_buf_mean": float(sb.mean()),
          "insert_success_buf_mean_of_the_groups_with_given_states": float(sb[real].mean()) if bool(real.any()) else None}
    path = _save(agent, save_to)
    tv = None
    if not fit:
        agent.ppo.close()
        task.sim.close()
        return None, path, st
    try:
        trn = TValue_Trainer.from_task(task, seed=seed)
        trn.init_TValue_function("BlockAssemblyInsertSim", fit_iters)
        # Only about 0.3 % of all brick orientations are ones InsertSim succeeds from.  The fit goes on (at most three more rounds) until it
        # rates at least 0.05 % of 20 000 random orientations above the chain's Orient gate: below that Orient's harvest can come out empty.
        g = torch.Generator().manual_seed(0)
        q = torch.randn(20000, 4, generator=g)
        q = (q / q.norm(dim=1, keepdim=True)).to(task.sim.device)
        rounds, cover = 0, 0.0
        while rounds < 4:
            trn.train_rollout()
            rounds += 1
            out = torch.cat([trn.predict(q[i:i + 1024]) for i in range(0, q.shape[0], 1024)])     # (sdxtv_predict takes at most one batch)
            cover = float((torch.sigmoid(out)[:, 1] > 0.5).float().mean())
            if cover >= 5e-4:
                break
        st["tvalue_fit"] = {"iterations": fit_iters * rounds, "loss": trn.losses[-1], "held_out_success_rate": trn.valid_t_value_success_rate,
                            "random_orientations_rated_above_0.5": cover}
        tv = flat_from_state_dict(trn.state_dict()).numpy()
        trn.close()
    except ValueError as ex:
        st["tvalue_fit"] = "skipped: %s" % ex
    agent.ppo.close()
    task.sim.close()
    return tv, path, st


def train_orient_policy(n, epochs, tvalue_state, gate=0.99, seed=22, save_to=None, minibatch=GRASP_TRAIN_MINIBATCH, initial_piles=None):
    """A BlockAssemblyOrient policy of THIS engine (round 6, VERDICT r5 item 6: the chain's Orient stage played a random initialisation):
    `epochs` epochs at n envs with the task's shipped schedule but 2 048-row minibatches (as train_grasp_policy; the shipped 4-row schedule
    does not learn on this engine), under the transition value `tvalue_state` binarised at `gate` (OR:1203: 0.99).
    Returns (checkpoint path or "", statistics: game reward, piles harvested per brick-type group, outcomes logged, mean T-value of the
    last step)."""
    task, env, agent = make_stage("BlockAssemblyOrient", n, seed, task_kwargs={"tvalue_gate": gate, "piles_per_type": 64, "initial_piles": initial_piles},
                                  minibatch_size=minibatch)
    task.sim.set_tvalue_weights(tvalue_state)
    wall, first = _train(agent, epochs)
    st = {"epochs": epochs, "minibatch_size": minibatch, "tvalue_gate": gate, "wall_s": wall, "game_reward_after_100_epochs": first,
          "game_reward": float(agent.game_rewards.get_mean()[0]), "game_length": float(agent.game_lengths.get_mean()[0]),
          "piles_harvested_per_type(during training)": task.sim.PILE_HARVEST_COUNT.cpu().tolist(),
          "outcomes_logged(success, failure)": task.sim.TV_COUNT.cpu().tolist(), "tvalue_mean_last_step": float(task.sim.TVALUE.mean()),
          "tvalue_max_last_step": float(task.sim.TVALUE.max())}
    path = _save(agent, save_to)
    agent.ppo.close()
    task.sim.close()
    return path, st


def tvalue_over_random_orientations(tvalue_state, count=200000, seed=0):
    """what a fitted GraspInsertTValue says about `count` uniformly random orientations (torch on the CPU; a statistic for reports):
    maximum and the shares above the gates the chain uses"""
    w = torch.from_numpy(np.asarray(tvalue_state, np.float32))
    off, x = 0, None
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(count, 4, generator=g)
    x = q / q.norm(dim=1, keepdim=True)
    for i, (_, out, inn) in enumerate(LAYERS):
        W = w[off:off + out * inn].view(out, inn); off += out * inn
        b = w[off:off + out]; off += out
        x = x @ W.t() + b
        if i < len(LAYERS) - 1:
            x = torch.relu(x)
    t = torch.sigmoid(x)[:, 1]
    return {"max": float(t.max()), "share_above_0.5": float((t > 0.5).float().mean()), "share_above_0.8": float((t > 0.8).float().mean()),
            "share_above_0.9": float((t > 0.9).float().mean()), "share_above_0.99": float((t > 0.99).float().mean())}


CHAIN_LEARNED_ORIENT_GATES = (0.99, 0.9, 0.8, 0.5, 0.3, 0.0)     # starts at the reference's threshold (OR:1203)


def block_assembly_chain_learned(num_envs=1024, grasp_epochs=1500, insert_epochs=1500, seed=22, workdir=None, min_grasp_states=1, max_grasp_steps=16000,
                                 insert_refit_epochs=4000):
    """BASELINE.json configs[2] on LEARNED policies (round 5) - no scripted stage, no synthetic grasp states:
      stage 0  BlockAssemblyInsertSim trains `insert_epochs` epochs with its shipped schedule from synthetic grasp states (the backward leg of
               bi_optimization.py:120-121 in small); GraspInsertTValue is fitted to its episode outcomes (thousands of successes since the
               studs engage) -> the transition value of the gates and the insert policy of the last stage;
      stage g  a BlockAssemblyGraspSim policy of this engine is trained `grasp_epochs` epochs (minibatch 2 048) with that transition value
               gating its harvest at the reference's 0.8 (GS:1406);
      stage r  (insert_refit_epochs > 0; the forward leg of the next bi-optimisation round, bi_optimization.py:115-118) the grasp policy is
               played from settled piles under the same gate, and the insert policy of stage 0 is fine-tuned on the states it harvested
               (brick-type groups without one keep synthetic states, named): a policy that has only seen synthetic hand poses inserts
               from 0.3 % of the learned grasp states, the fine-tuned one from several per cent;
      chain    Orient (random-initialised policy - its arm is scripted by the task - under a ladder of gates that starts at the reference's 0.99;
               the rung used is reported; a group it harvests nothing for starts GraspSim from settled piles, named in the statistics) ->
               GraspSim (the learned policy, gate 0.8, played until every brick-type group has `min_grasp_states` harvested states) ->
               InsertSim (the learned insert policy, started from those states only: a group without one raises, as IS:1449 fails).
    Returns (statistics, hand-off tensors; the caller closes hand["insert_task"].sim)."""
    workdir = workdir or tempfile.mkdtemp(prefix="sdx_chain_learned_")
    tv, ipath, ist = prepare_tvalue_and_insert_policy(num_envs, insert_epochs, seed=seed, save_to=os.path.join(workdir, "insert"))
    if tv is None:
        raise RuntimeError("stage 0 logged too few insert outcomes of a class for a transition value: %s" % ist)
    gpath, gtask, gst = train_grasp_policy(num_envs, grasp_epochs, seed=seed, save_to=os.path.join(workdir, "grasp"), tvalue_state=tv)
    gtask.sim.close()
    rst = None
    if insert_refit_epochs > 0:
        g0, st0 = main_rlgames("BlockAssemblyGraspSim", num_envs, policy_path=gpath, tvalue_state=tv, steps=160, seed=seed + 1,
                               until=lambda t: int(t.sim.HARVEST_COUNT.min()) >= 64, max_steps=max_grasp_steps, task_kwargs={"harvest_tvalue_gate": 0.8})
        cnt0 = g0.sim.HARVEST_COUNT.cpu().tolist()
        if max(cnt0) > 0:
            s0 = g0.grasp_terminal_states()
            g0.sim.close()
            _, ipath, rst = prepare_tvalue_and_insert_policy(num_envs, insert_refit_epochs, seed=seed, save_to=os.path.join(workdir, "insert_refit"),
                                                             grasp_states=s0, restore=ipath, synthetic_fallback=True, fit=False)
            rst["grasp_states_harvested_per_type(settled piles, gate 0.8, %d steps per env)" % st0["steps_per_env"]] = cnt0
        else:
            g0.sim.close()
            rst = {"skipped": "the grasp policy harvested no state under gate 0.8 in %d steps per env" % st0["steps_per_env"]}
    res, hand = block_assembly_chain(num_envs, tv, policies={"grasp": gpath, "insert": ipath}, synthetic_fallback=False, orient_fallback=True,
                                     orient_tvalue_gate=CHAIN_LEARNED_ORIENT_GATES, grasp_tvalue_gate=0.8, stage_steps={"grasp": 160},
                                     min_grasp_states=min_grasp_states, max_grasp_steps=max_grasp_steps, seed=seed)
    out = {"stage0_insert_policy_and_tvalue(untimed)": ist, "grasp_policy(untimed)": gst, "insert_policy_refit(untimed)": rst, "chain": res,
           "stand_ins": ["Orient plays its random initialisation under T-value gate %s (reference: a trained Orient policy under 0.99)" % res["orient"]["tvalue_gate"]]
           + (["settled piles for Orient's brick-type groups %s" % res["orient"]["settled_stand_in_groups"]] if res["orient"].get("settled_stand_in_groups") else [])}
    return out, hand


def block_assembly_chain_closed(num_envs=1024, insert_epochs=1500, grasp_epochs=1500, insert_refit_epochs=4000, orient_epochs=600, seed=22, workdir=None,
                                min_grasp_states=100, max_grasp_steps=16000, orient_gates=(0.99,), refit_harvest_per_type=100, grasp_gates=(0.8,)):
    """The chain with EVERY stage on a learned policy and the transition value refitted to the policy that actually ends the chain
    (round 6; scripts/evaluation.py:111-119 on the output of one forward + backward pass of scripts/bi_optimization.py:110-124):
      stage 0  BlockAssemblyInsertSim trains from synthetic grasp states; GraspInsertTValue is fitted to its outcomes (as the learned chain);
      stage g  a GraspSim policy is trained under that value's gate 0.8 (GS:1406);
      stage r  the grasp policy is played from settled piles until every brick-type group has `refit_harvest_per_type` harvested states
               (round 5 took 64 and the chain itself handed on 32 states in all: VERDICT r5 item 5c), the insert policy is fine-tuned on them AND
               the transition value is REFITTED to the fine-tuned policy's outcomes (the value the backward legs of the loop hand to GraspSim
               and Orient, bi_optimization.py:121-124);
      stage o  a BlockAssemblyOrient policy is TRAINED under the refitted value (round 5: random initialisation);
      chain    Orient (trained; gate ladder `orient_gates`, default the reference's 0.99 alone) -> GraspSim (trained, gate 0.8, until every group
               has `min_grasp_states` states) -> InsertSim (fine-tuned).
    Returns (statistics, hand-off tensors; the caller closes hand["insert_task"].sim)."""
    workdir = workdir or tempfile.mkdtemp(prefix="sdx_chain_closed_")
    tv0, ipath, ist = prepare_tvalue_and_insert_policy(num_envs, insert_epochs, seed=seed, save_to=os.path.join(workdir, "insert"))
    if tv0 is None:
        raise RuntimeError("stage 0 logged too few insert outcomes of a class for a transition value: %s" % ist)
    gpath, gtask, gst = train_grasp_policy(num_envs, grasp_epochs, seed=seed, save_to=os.path.join(workdir, "grasp"), tvalue_state=tv0)
    gtask.sim.close()
    # the harvest gate: GS:1406's 0.8 first; `grasp_gates` may continue with lower rungs for the seeds whose stage-0 value rates every
    # grasp of some brick type below 0.8 (two of three seeds in profiles/r6_chain_closed_seeds_22_23_24_first_attempt.json) - a rung
    # below 0.8 is reported as a stand-in
    tried0 = []
    for gi, gate0 in enumerate(grasp_gates):
        g0, st0 = main_rlgames("BlockAssemblyGraspSim", num_envs, policy_path=gpath, tvalue_state=tv0, steps=160, seed=seed + 1,
                               until=lambda t: int(t.sim.HARVEST_COUNT.min()) >= refit_harvest_per_type, max_steps=max_grasp_steps,
                               task_kwargs={"harvest_tvalue_gate": gate0})
        cnt0 = g0.sim.HARVEST_COUNT.cpu().tolist()
        tried0.append({"tvalue_gate": gate0, "grasp_states_harvested_per_type": cnt0, "steps_per_env": st0["steps_per_env"]})
        if min(cnt0) > 0 or gi + 1 == len(grasp_gates):
            break
        g0.sim.close()
    if min(cnt0) == 0:
        g0.sim.close()
        raise RuntimeError("the grasp policy harvested no state for a brick-type group under the gates %s in %d steps per env: %s" % (list(grasp_gates), st0["steps_per_env"], cnt0))
    s0 = g0.grasp_terminal_states()
    g0.sim.close()
    tv1, ipath1, rst = prepare_tvalue_and_insert_policy(num_envs, insert_refit_epochs, seed=seed, save_to=os.path.join(workdir, "insert_refit"),
                                                        grasp_states=s0, restore=ipath, synthetic_fallback=False, fit=True)
    rst["grasp_states_harvested_per_type(settled piles, gate %s, %d steps per env)" % (gate0, st0["steps_per_env"])] = cnt0
    rst["refit_harvest_gates_tried"] = tried0
    tv = tv1 if tv1 is not None else tv0
    tvs = {"stage0": tvalue_over_random_orientations(tv0), "refitted": tvalue_over_random_orientations(tv1) if tv1 is not None else None,
           "used_by_the_chain": "refitted to the fine-tuned insert policy" if tv1 is not None else "stage 0 (the refit was skipped: %s)" % rst.get("tvalue_fit")}
    opath, ost = train_orient_policy(num_envs, orient_epochs, tv, gate=orient_gates[0], seed=seed, save_to=os.path.join(workdir, "orient"))
    res, hand = block_assembly_chain(num_envs, tv, policies={"orient": opath, "grasp": gpath, "insert": ipath1}, synthetic_fallback=False, orient_fallback=True,
                                     orient_tvalue_gate=tuple(orient_gates), grasp_tvalue_gate=tuple(grasp_gates), stage_steps={"grasp": 160},
                                     min_grasp_states=min_grasp_states, max_grasp_steps=max_grasp_steps, seed=seed)
    stand_ins = []
    if gate0 != 0.8:
        stand_ins.append("refit harvest of grasp states under gate %s instead of 0.8 (GS:1406)" % gate0)
    if res["grasp"]["tvalue_gate"] != 0.8:
        stand_ins.append("the chain's GraspSim stage under gate %s instead of 0.8 (GS:1406)" % res["grasp"]["tvalue_gate"])
    if res["orient"]["tvalue_gate"] != 0.99:
        stand_ins.append("Orient's gate %s instead of 0.99 (the ladder's first rung that harvested)" % res["orient"]["tvalue_gate"])
    if res["orient"].get("settled_stand_in_groups"):
        stand_ins.append("settled piles for Orient's brick-type groups %s" % res["orient"]["settled_stand_in_groups"])
    out = {"stage0_insert_policy_and_tvalue(untimed)": ist, "grasp_policy(untimed)": gst, "insert_policy_refit_and_tvalue_refit(untimed)": rst,
           "orient_policy(untimed)": ost, "tvalue_over_200000_random_orientations": tvs, "chain": res, "stand_ins": stand_ins}
    return out, hand
