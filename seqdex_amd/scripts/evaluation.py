"""Chained evaluation of the BlockAssembly sub-policies, after the reference's scripts/evaluation.py:36-119: every stage is played (no
update) with the transition value switched on, and leaves the terminal states the next stage starts from:

    BlockAssemblyOrient    --pile states of episodes that end with the target brick reachable (OR:1463-1488)-->
    BlockAssemblyGraspSim  --grasp terminal states: brick carried to the insertion side, still in the hand, T-value > 0.8 (GS:1404-1417)-->
    BlockAssemblyInsertSim   (every reset draws the brick and the hand from those states, IS:372-375,1449-1456)

Where the reference hands the states over through pickles under ./intermediate_state/, the stages here hand over device tensors with the
same content (the pickle forms exist too: seqdex_amd/piles.py, BlockAssemblyGraspSim.save_grasp_terminal_states).  BASELINE.json
configs[2] is this chain at num_envs = 1024 on one GPU; tools/bench_config3.py times it, tests/test_gpu_chain.py checks the hand-offs.

    python -m seqdex_amd.scripts.evaluation --tasks BlockAssembly [--num_envs 512] [--search s.pth] --orient o.pth --grasp g.pth --insert i.pth [--games 512]
    python -m seqdex_amd.scripts.evaluation --mode chain_learned [--num_envs 1024]
    python -m seqdex_amd.scripts.evaluation --mode chain [--tvalue tv.pt] [--synthetic_fallback --orient_tvalue_gate 0.5 --grasp_tvalue_gate 0.28]
"""
import argparse
import time

import numpy as np
import torch

from ..stage import make_stage

# Orient's T-value gate in the chain benchmark / test when the transition value comes from a stage 0 of a thousand epochs: a descending
# ladder, the last rung opens the gate (block_assembly_chain, stage 1).  The reference's threshold is 0.99 (OR:1203).
CHAIN_ORIENT_GATES = (0.5, 0.4, 0.3, 0.28, 0.0)
CHAIN_GRASP_GATES = (0.28, 0.0)         # GraspSim's harvest gate in the same setting (reference: 0.8, GS:1406)


def main_rlgames(task, num_envs, play=True, use_t_value=True, policy_path="", steps=None, task_kwargs=None, tvalue_state=None,
                 controller=None, seed=22, until=None, max_steps=None):
    """one stage of scripts/evaluation.py:36-103: build the task and its agent, restore `policy_path`, play.  `steps` env steps are
    played in horizon-sized chunks (default: one episode + its reset); `until(task)` may end the stage earlier / later (checked after
    every chunk, at most `max_steps`).  `controller(task, step) -> actions [N, 23]` replaces the policy (a scripted stand-in; the
    returned statistics say so).  Returns (task object - the caller closes task.sim -, statistics)."""
    assert play, "the chain evaluation only plays"
    # seeded as the launcher seeds every run (TR:70, CF:35-59): RLgamesVecTaskPython.reset draws its noise step from torch's global generator
    t_obj, env, agent = make_stage(task, num_envs, seed, play=True, task_kwargs=task_kwargs, config_overrides={"name": task}, restore=policy_path)
    if tvalue_state is not None and use_t_value:
        t_obj.sim.set_tvalue_weights(tvalue_state)
    horizon = agent.horizon_length
    if steps is None:
        steps = int(t_obj.max_episode_length) + horizon
    max_steps = max_steps or steps
    deterministic = bool(agent.config.get("player", {}).get("deterministic", True))
    torch.cuda.synchronize()
    t0 = time.time()
    done = 0
    if controller is not None:
        env.reset()
    while done < max_steps:
        if controller is None:
            agent.play_steps(deterministic)
        else:
            for _ in range(horizon):
                env.step(controller(t_obj, done + _))
        done += horizon
        if done >= steps and (until is None or until(t_obj)):
            break
    torch.cuda.synchronize()
    dt = time.time() - t0
    stats = {"task": task, "num_envs": num_envs, "env_steps": done * num_envs, "steps_per_env": done, "wall_s": dt,
             "env_steps_per_s": done * num_envs / dt, "policy": (policy_path or "random initialisation (seed %d)" % seed) if controller is None
             else "scripted stand-in controller (%s)" % getattr(controller, "__name__", "callable"),
             "success_buf_mean": float(t_obj.extras["success_buf"].float().mean())}
    agent.ppo.close()
    return t_obj, stats


def fill_missing_pile_groups(harvest, counts, min_piles, seed, max_missing=2, keys=None):
    """Brick-type groups Orient could not fill (the gate of a briefly fitted T-value can miss the orientations one brick type settles in)
    start GraspSim from settled piles instead - the states GraspSim generates for itself when it is given none (piles.generate_piles) - as
    InsertSim's groups without a harvested grasp state fall back to its synthetic ones.  harvest [8, slots, 132, 13], counts [8].
    Returns ([8, K, 132, 13], the groups that were filled in) or (None, []) when every group has min_piles or more than max_missing lack them."""
    from ..piles import generate_piles
    cnt = np.minimum(counts.cpu().numpy(), harvest.shape[1])
    lacking = [t for t in range(8) if cnt[t] < min_piles]
    if not lacking or len(lacking) > max_missing:
        return None, []
    k = int(cnt[cnt >= min_piles].min())
    piles = harvest[:, :k].clone()
    if keys is not None:                                   # serial (step, env) order of the appends, as pile_terminal_states() hands them on
        for t in range(8):
            if cnt[t] >= k:
                piles[t] = harvest[t, :int(cnt[t])].index_select(0, torch.argsort(keys[t, :int(cnt[t])], stable=True))[:k]
    settled = torch.as_tensor(generate_piles(k, device=str(piles.device), seed=seed)).to(piles.device)
    for t in lacking:
        piles[t] = settled[t]
    return piles, lacking


def block_assembly_chain(num_envs=512, tvalue_state=None, policies=None, controllers=None, min_piles=8, seed=22, stage_steps=None,
                         synthetic_fallback=False, orient_tvalue_gate=0.99, grasp_tvalue_gate=0.8, with_search=False, min_grasp_states=0,
                         max_grasp_steps=None, orient_fallback=None):
    """Orient -> GraspSim -> InsertSim played back to back on one GPU.  policies / controllers / stage_steps: dicts keyed "orient",
    "grasp", "insert".  Orient plays until every brick-type group has `min_piles` harvested pile states (OR:1483-1488 fills rings of
    10 000; at most 8 episodes here).  orient_tvalue_gate: the threshold Orient binarises the transition value at (0.99, OR:1203), or
    a descending ladder of thresholds (see stage 1 below); a T-value fitted to a few hundred epochs of outcomes never gets that
    confident, so the chain benchmark lowers it (and GraspSim's 0.8, GS:1406) and says so.
    min_grasp_states > 0: GraspSim plays (in horizon-sized chunks, at most max_grasp_steps env steps) until every brick-type group has that
    many harvested grasp states - a learned grasp policy under the reference's gate 0.8 harvests a state every few dozen episodes.
    orient_fallback: overrides synthetic_fallback for Orient's hand-off only (settled piles for the groups Orient harvested nothing for).
    Returns (statistics, hand-off tensors for inspection)."""
    orient_fallback = synthetic_fallback if orient_fallback is None else orient_fallback
    policies, controllers, stage_steps = policies or {}, controllers or {}, stage_steps or {}
    out, hand = {"num_envs": num_envs, "min_piles_per_type": min_piles}, {}
    t_begin = time.time()
    dug = None
    if with_search:
        # ---- stage 0: BlockAssemblySearch at <= 128 envs (evaluation.py:111): piles whose target brick the camera sees go to Orient (SE:1323-1353)
        search, st = main_rlgames("BlockAssemblySearch", min(num_envs, 128), policy_path=policies.get("search", ""), seed=seed,
                                  controller=controllers.get("search"), steps=stage_steps.get("search", 2 * (75 + 8)))
        st["piles_harvested_per_type"] = search.sim.PILE_HARVEST_COUNT.cpu().tolist()
        dug = search.pile_terminal_states()
        if dug is not None and dug.shape[1] < 8:      # too few states to start 128 envs per group from: Orient would replay the same handful
            st["handed_on"] = "only %d piles per group (< 8): Orient settles its own piles" % dug.shape[1]
            dug = None
        else:
            st["handed_on"] = "none (a brick-type group has no dug-out pile): Orient settles its own piles" if dug is None else "%d piles per group" % dug.shape[1]
        search.sim.close()
        out["search"] = st
    # ---- stage 1: BlockAssemblyOrient.  orient_tvalue_gate may be a descending ladder of thresholds: Orient is replayed at the next rung
    # when a rung leaves more brick-type groups without piles than the settled-pile fallback covers.  What a briefly fitted transition
    # value accepts depends on which few orientations its training run happened to succeed from (stage 0 is deterministic for one build
    # of the library, but any change of a summation order moves it), so a fixed lowered gate can come out empty; the last rung 0.0
    # opens the gate.  The rung used and the rungs tried are in the statistics; only the run that was handed on is timed.
    ladder = list(orient_tvalue_gate) if isinstance(orient_tvalue_gate, (tuple, list)) else [orient_tvalue_gate]
    tried, probe_wall = [], 0.0
    for gate in ladder:
        orient, st = main_rlgames("BlockAssemblyOrient", num_envs, policy_path=policies.get("orient", ""), tvalue_state=tvalue_state,
                                  controller=controllers.get("orient"), seed=seed, steps=stage_steps.get("orient"),
                                  until=lambda t: int(t.sim.PILE_HARVEST_COUNT.min()) >= min_piles,
                                  max_steps=8 * 80 if stage_steps.get("orient") is None else stage_steps["orient"],
                                  task_kwargs={"tvalue_gate": gate, "piles_per_type": 64, "initial_piles": dug})
        st["piles_harvested_per_type"] = orient.sim.PILE_HARVEST_COUNT.cpu().tolist()
        st["tvalue_gate"] = gate
        piles = orient.pile_terminal_states()
        if orient_fallback:
            filled, lacking = fill_missing_pile_groups(orient.sim.PILE_HARVEST, orient.sim.PILE_HARVEST_COUNT, min_piles, seed, keys=orient.sim.PILE_HARVEST_KEYS)
            if lacking:
                piles, st["settled_stand_in_groups"] = filled, lacking
        orient.sim.close()
        tried.append({"tvalue_gate": gate, "piles_harvested_per_type": st["piles_harvested_per_type"]})
        if piles is not None:
            break
        probe_wall += st["wall_s"]
    if len(ladder) > 1:
        st["tvalue_gates_tried"], st["wall_s_of_the_rungs_not_handed_on"] = tried, probe_wall
    out["orient"] = st
    if piles is None:
        raise RuntimeError("BlockAssemblyOrient harvested no pile state for at least one brick-type group: %s" % st["piles_harvested_per_type"])
    hand["piles"] = piles
    # ---- stage 2: BlockAssemblyGraspSim from Orient's piles (GS:412-413).  grasp_tvalue_gate may be a ladder like Orient's: the next rung
    # is played when a rung harvests grasp states for fewer than three brick-type groups.
    gladder = list(grasp_tvalue_gate) if isinstance(grasp_tvalue_gate, (tuple, list)) else [grasp_tvalue_gate]
    gtried, gprobe = [], 0.0
    for gi, gate in enumerate(gladder):
        grasp, st = main_rlgames("BlockAssemblyGraspSim", num_envs, policy_path=policies.get("grasp", ""), tvalue_state=tvalue_state,
                                 controller=controllers.get("grasp"), seed=seed, steps=stage_steps.get("grasp"),
                                 until=(lambda t: int(t.sim.HARVEST_COUNT.min()) >= min_grasp_states) if min_grasp_states > 0 else None,
                                 max_steps=max_grasp_steps,
                                 task_kwargs={"initial_piles": piles, "harvest_tvalue_gate": gate})
        cnt = grasp.sim.HARVEST_COUNT.cpu().numpy()
        gtried.append({"tvalue_gate": gate, "grasp_states_harvested_per_type": cnt.tolist()})
        # (next rung: fewer than three groups harvested - or, when no stand-in states are allowed, any group without a state)
        if (int((cnt > 0).sum()) >= 3 and (synthetic_fallback or cnt.min() > 0)) or gi + 1 == len(gladder):
            break
        gprobe += st["wall_s"]
        grasp.sim.close()
    st["tvalue_gate"] = gate
    if len(gladder) > 1:
        st["tvalue_gates_tried"], st["wall_s_of_the_rungs_not_handed_on"] = gtried, gprobe
    st["grasp_states_harvested_per_type"] = cnt.tolist()
    st["initial_piles"] = "BlockAssemblyOrient.pile_terminal_states(): %d per brick-type group" % piles.shape[1]
    if cnt.min() > 0 or (synthetic_fallback and cnt.max() > 0):
        grasp_states = grasp.grasp_terminal_states()          # (groups without a harvested state: empty tensors -> InsertSim's stand-ins)
        hand["grasp_obj"], hand["grasp_hand"] = grasp_states
    elif synthetic_fallback:
        grasp_states = None
    else:
        grasp.sim.close()
        out["grasp"] = st
        raise RuntimeError("BlockAssemblyGraspSim harvested no grasp terminal state for at least one brick-type group: %s" % cnt.tolist())
    grasp.sim.close()
    out["grasp"] = st
    # ---- stage 3: BlockAssemblyInsertSim from the harvested grasp states (IS:372-375)
    insert, st = main_rlgames("BlockAssemblyInsertSim", num_envs, policy_path=policies.get("insert", ""), tvalue_state=tvalue_state,
                              controller=controllers.get("insert"), seed=seed, steps=stage_steps.get("insert"),
                              task_kwargs={"grasp_states": grasp_states, "synthetic_fallback": synthetic_fallback})
    st["grasp_states_source"] = insert.grasp_states_source
    hand["insert_task"] = insert          # the caller inspects it and closes insert.sim
    out["insert"] = st
    out["chain_wall_s"] = time.time() - t_begin
    stages = [k for k in ("search", "orient", "grasp", "insert") if k in out]
    steps = sum(out[k]["env_steps"] for k in stages)
    play = sum(out[k]["wall_s"] for k in stages)
    out["chain_env_steps"] = steps
    out["chain_env_steps_per_s"] = steps / play                      # the three rollouts back to back (task construction excluded)
    out["chain_env_steps_per_s_incl_setup"] = steps / out["chain_wall_s"]
    return out, hand


# ---------------------------------------------------------------------------------------------------------------------------------
# the checkpoint-driven form (round 2): every stage through the launcher's own argument parsing, optional BlockAssemblySearch stage first
def _launcher():
    from ..config import get_args
    from ..train_rlgames import build
    return get_args, build


def play_checkpoint(task, num_envs, play=True, use_t_value=False, policy_path="", games=0, task_kwargs=None, minibatch_size=0):
    """evaluation.py:36-103 for one stage through the reference's command line (--task --num_envs --checkpoint --play; seqdex_amd.train_rlgames.build):
    the sub-policy is restored from its checkpoint and played for `games` finished episodes.  Returns (mean episode reward, mean episode length, task object)."""
    argv = ["--task=%s" % task, "--num_envs=%d" % num_envs, "--headless", "--play"]
    if policy_path:
        argv.append("--checkpoint=%s" % policy_path)
    get_args, build = _launcher()
    args = get_args(argv)
    args.use_t_value = use_t_value
    task_obj, env, agent, logdir, rank = build(args, task_kwargs, minibatch_size)
    agent.play(games or num_envs)
    torch.cuda.synchronize()
    rew, length = float(agent.game_rewards.get_mean()[0]), float(agent.game_lengths.get_mean()[0])
    agent.ppo.close()
    return rew, length, task_obj


def block_assembly(orient_path, grasp_path, insert_path, num_envs=512, games=0, insert_minibatch=0, search_path=None):
    out = {}
    dug = None
    if search_path is not None:
        r, l, search = play_checkpoint("BlockAssemblySearch", min(num_envs, 128), use_t_value=True, policy_path=search_path, games=games)
        dug = search.pile_terminal_states()
        out["BlockAssemblySearch"] = dict(reward=r, length=l, search_success_rate=float(search.extras["success_buf"].float().mean()),
                                          piles_handed_on=0 if dug is None else int(dug.shape[1]))
        search.sim.close()
    r, l, orient = play_checkpoint("BlockAssemblyOrient", num_envs, use_t_value=True, policy_path=orient_path, games=games,
                                task_kwargs={"initial_piles": dug})
    piles = orient.pile_terminal_states()
    out["BlockAssemblyOrient"] = dict(reward=r, length=l, piles_handed_on=0 if piles is None else int(piles.shape[1]))
    orient.sim.close()
    r, l, grasp = play_checkpoint("BlockAssemblyGraspSim", num_envs, use_t_value=True, policy_path=grasp_path, games=games,
                               task_kwargs={"initial_piles": piles})
    cnt = grasp.sim.HARVEST_COUNT.cpu().numpy()
    states = grasp.grasp_terminal_states() if cnt.min() > 0 else None
    out["BlockAssemblyGraspSim"] = dict(reward=r, length=l, grasp_states_handed_on=int(cnt.sum()))
    grasp.sim.close()
    r, l, insert = play_checkpoint("BlockAssemblyInsertSim", num_envs, use_t_value=True, policy_path=insert_path, games=games,
                                task_kwargs={"grasp_states": states}, minibatch_size=insert_minibatch)
    out["BlockAssemblyInsertSim"] = dict(reward=r, length=l, insert_success_rate=float(insert.extras["success_buf"].float().mean()),
                                         grasp_states=insert.grasp_states_source)
    insert.sim.close()
    for k, v in out.items():
        print(k, v)
    return out


if __name__ == "__main__":
    p = argparse.ArgumentParser(description="scripts/evaluation.py of the reference: play the BlockAssembly sub-policies back to back")
    p.add_argument("--tasks", type=str, default="BlockAssembly")
    p.add_argument("--mode", choices=["checkpoint", "chain", "chain_learned"], default="checkpoint",
                   help="checkpoint: every stage restored from its rl_games .pth through the launcher and played for --games episodes "
                        "(evaluation.py:111-119; a stage without a checkpoint plays its random initialisation); chain: the device-tensor "
                        "hand-off chain of block_assembly_chain with the harvest gates below; chain_learned: chain_training.block_assembly_chain_learned "
                        "(trains the insert policy, the transition value and a grasp policy and fine-tunes the insert policy first: under three minutes at 1 024 envs)")
    p.add_argument("--num_envs", type=int, default=512)
    for st_ in ("search", "orient", "grasp", "insert"):
        p.add_argument("--%s" % st_, "--%s_policy" % st_, dest=st_, type=str, default="", help="rl_games checkpoint (.pth) of the %s stage" % st_)
    p.add_argument("--with_search", action="store_true", help="put BlockAssemblySearch (128 envs) in front (always on in checkpoint mode when --search is given)")
    p.add_argument("--games", type=int, default=0, help="checkpoint mode: finished episodes per stage (0 = num_envs)")
    p.add_argument("--insert_minibatch", type=int, default=0)
    p.add_argument("--tvalue", type=str, default="", help="chain mode: GraspInsertTValue state_dict (.pt) for the harvest gates")
    p.add_argument("--synthetic_fallback", action="store_true", help="chain mode: brick-type groups a stage harvested nothing for start the next "
                   "stage from settled piles / synthetic grasp states (named in the statistics) instead of failing as the reference does")
    p.add_argument("--orient_tvalue_gate", type=float, nargs="+", default=[0.99], help="OR:1203; several values = a descending ladder (block_assembly_chain)")
    p.add_argument("--grasp_tvalue_gate", type=float, nargs="+", default=[0.8], help="GS:1406; several values = a ladder")
    a = p.parse_args()
    if a.tasks != "BlockAssembly":
        raise Exception("Unrecognized task!")                        # evaluation.py:121-129 (ToolPositioning: not built)
    if a.mode == "chain_learned":
        import json
        from .chain_training import block_assembly_chain_learned
        res, h = block_assembly_chain_learned(a.num_envs)
        h["insert_task"].sim.close()
        print(json.dumps(res))
    elif a.mode == "checkpoint":
        block_assembly(a.orient, a.grasp, a.insert, num_envs=a.num_envs, games=a.games, insert_minibatch=a.insert_minibatch,
                       search_path=a.search if (a.search or a.with_search) else None)
    else:
        tv = None
        if a.tvalue:
            from ..tvalue_trainer import flat_from_state_dict
            tv = flat_from_state_dict(torch.load(a.tvalue, map_location="cpu")).numpy()
        res, h = block_assembly_chain(a.num_envs, tv, {"search": a.search, "orient": a.orient, "grasp": a.grasp, "insert": a.insert},
                                      synthetic_fallback=a.synthetic_fallback, orient_tvalue_gate=a.orient_tvalue_gate[0] if len(a.orient_tvalue_gate) == 1 else a.orient_tvalue_gate,
                                      grasp_tvalue_gate=a.grasp_tvalue_gate[0] if len(a.grasp_tvalue_gate) == 1 else a.grasp_tvalue_gate, with_search=a.with_search)
        h["insert_task"].sim.close()
        import json
        print(json.dumps(res))
