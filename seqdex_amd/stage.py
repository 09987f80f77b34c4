"""One way to build a stage of the BlockAssembly chain: the task, its rl_games-facing wrapper and the agent, from the shipped YAMLs
(what utils/parse_task.py:162-178 and train_rlgames.py:78-94 do for the reference's launcher).  The chain scripts, the tools and the
launcher (train_rlgames.build) all come through here, so a new construction argument is threaded through one place.

Order is behaviour: RLgamesVecTaskPython.reset draws its noise step from torch's global generator and the task constructors draw from
generators seeded with `seed`, so make_stage seeds first and then builds task, wrapper, agent in that order."""
import importlib

from .config import set_seed, task_cfg, train_cfg

TASK_MODULES = {"BlockAssemblyGraspSim": "block_assembly_grasp_sim", "BlockAssemblyOrient": "block_assembly_orient",
                "BlockAssemblyInsertSim": "block_assembly_insert_sim", "BlockAssemblySearch": "block_assembly_search"}   # keys == config.TASK_CFG's


def task_class(name):
    """task name -> task class (eval(args.task), PT:162); the module is imported on first use"""
    return getattr(importlib.import_module("seqdex_amd.tasks." + TASK_MODULES[name]), name)


def make_task(name, num_envs, seed=22, play=False, cfg=None, **task_kwargs):
    """the task `name` at `num_envs` envs on cuda:0 from its shipped YAML (cfg: that YAML already loaded, for a caller that edits it
    first).  Seeds nothing global: a caller that goes on to RLgamesVecTaskPython.reset() seeds torch itself (make_stage does)."""
    cfg = task_cfg(name) if cfg is None else cfg
    cfg["env"]["numEnvs"] = num_envs
    if play:
        cfg["env"]["test"] = True                                                         # TR:68
    return task_class(name)(cfg, device_type="cuda", device_id=0, headless=True, seed=seed, **task_kwargs)


def wrap_and_build_agent(task, cfg_train, seed, rl_device="cuda:0", minibatch_size=0, config_overrides=None, restore=""):
    """task + rl_games YAML dict -> (env, agent).  minibatch_size != 0 replaces the policy's and the central value's (the reference parses
    --minibatch_size but never applies it, CF:43); config_overrides: keys written into params.config before the agent is built; restore:
    a checkpoint to go on from, its epoch counter reset (the caller trains or plays MORE epochs; rl_games would resume the counter)."""
    from .a2c_agent import A2CAgent
    from .vec_task_rlgames import RLgamesVecTaskPython
    env = RLgamesVecTaskPython(task, rl_device)                                           # PT:178
    pc = cfg_train["params"]["config"]                                                    # TR:78-85
    if minibatch_size:
        pc["minibatch_size"] = minibatch_size
        pc["central_value_config"]["minibatch_size"] = minibatch_size
    pc.update(config_overrides or {})
    pc.update(num_actors=env.num_environments, vec_env=env, env_info=env.get_env_info(), seed=seed)
    agent = A2CAgent("run", cfg_train["params"])                                          # TR:88-94
    if restore:
        agent.restore(restore)
        agent.epoch_num = 0
    return env, agent


def make_stage(name, num_envs, seed=22, *, play=False, task_kwargs=None, minibatch_size=0, config_overrides=None, restore=""):
    """-> (task, env, agent) of the stage `name`, seeded as the launcher seeds a run (TR:70, CF:35-59).  The caller closes agent.ppo and
    task.sim."""
    set_seed(seed)
    task = make_task(name, num_envs, seed, play, **(task_kwargs or {}))
    env, agent = wrap_and_build_agent(task, train_cfg(name), seed, minibatch_size=minibatch_size, config_overrides=config_overrides, restore=restore)
    return task, env, agent
