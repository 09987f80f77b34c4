"""Launcher with the reference's command line (train_rlgames.py:33-94):

    python -m seqdex_amd.train_rlgames --task=BlockAssemblyGraspSim --num_envs=1024 [--seed 22] [--max_iterations N]
                                       [--checkpoint path --play]          # one process per GPU under torchrun

args -> cfg (utils/config.py semantics) -> task + VecTask adapter (utils/parse_task.py:162-178) -> A2CAgent (the
rl_games Runner is replaced by seqdex_amd.a2c_agent, same YAML schema)."""
import os


def build(args, task_kwargs=None, minibatch_size=0, config_overrides=None):
    """args (config.get_args) -> (task, env, agent, logdir, rank): everything main() does before agent.train() / agent.play().
    config_overrides: keys written into the YAML's params.config before the agent is built (e.g. mixed_precision: True, rl_games' own key)"""
    import torch
    from .config import load_cfg, set_seed
    from .stage import task_class, wrap_and_build_agent
    args.algo = "lego"                                                                    # TR:36
    args.task_type = "RLgames"                                                            # TR:56
    print("Loading config: ", args.cfg_train)
    cfg, cfg_train, logdir = load_cfg(args)
    seed = args.seed if args.seed is not None else 22                                     # TR:62-65
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(args.device_id)))
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))       # RCCL over xGMI
    cfg["env"]["test"] = args.play                                                        # TR:68
    set_seed(seed + rank, args.torch_deterministic)                                       # TR:70 (+ rank, App. C)
    task = task_class(args.task)(cfg, None, None, "cuda", local_rank, True, seed=seed + rank, **(task_kwargs or {}))   # PT:162-170
    cfg_train["params"]["seed"] = seed                                                    # TR:78-85 (the agent adds the rank itself)
    cfg_train["params"]["config"]["env_config"]["seed"] = seed
    env, agent = wrap_and_build_agent(task, cfg_train, seed, args.rl_device, minibatch_size,
                                      {**(config_overrides or {}), "name": args.task, "multi_gpu": world > 1})
    if getattr(args, "record", ""):                # frames of the chosen envs after every env step (view.Recorder), rank 0 only
        from .view import Recorder
        if rank == 0:
            env.recorder = Recorder(task, args.record, args.record_envs, args.record_every, args.record_camera, args.record_size)
    if cfg_train["params"].get("load_path"):       # (resumes the checkpoint's epoch counter, as rl_games does)
        agent.restore(cfg_train["params"]["load_path"])
    return task, env, agent, logdir, rank


def main(argv=None):
    from .config import get_args
    args = get_args(argv)
    task, env, agent, logdir, rank = build(args)
    if args.train:
        agent.train()
        if rank == 0:
            os.makedirs(os.path.join(logdir, "nn"), exist_ok=True)
            agent.save(os.path.join(logdir, "nn", "last_%s_ep_%d" % (args.task, agent.epoch_num)))
    else:
        agent.play(int(agent.config.get("player", {}).get("games_num", 1)))


if __name__ == "__main__":
    main()
