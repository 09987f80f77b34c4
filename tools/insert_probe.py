"""How well does BlockAssemblyInsertSim train on this engine?  N envs, shipped schedule (minibatch 4096), `epochs` epochs from synthetic grasp
states (or --grasp: from the states a freshly trained grasp policy harvested); prints the outcome counts and, every `every` epochs, the
distribution of the distance / rotation error to the insertion site (SDX_T_INSERT_AUX) over the envs.
usage: python tools/insert_probe.py N epochs every [--grasp GE] [--no-hollow]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seqdex_amd.stage import make_stage  # noqa: E402
from seqdex_amd.tasks.block_assembly_insert_sim import BlockAssemblyInsertSim  # noqa: E402

n, epochs, every = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
states = None
if "--grasp" in sys.argv:
    from seqdex_amd.scripts.chain_training import train_grasp_policy
    ge = int(sys.argv[sys.argv.index("--grasp") + 1])
    _, gtask, gst = train_grasp_policy(n, ge, seed=22)
    states = gtask.grasp_terminal_states()
    gtask.sim.close()
    print("grasp policy:", json.dumps(gst), flush=True)
if "--no-hollow" in sys.argv:       # patched on the class itself: make_stage builds the task by name
    hollow = BlockAssemblyInsertSim._scene_overrides
    BlockAssemblyInsertSim._scene_overrides = lambda self, scene: dict(hollow(self, scene), seg_hollow=0)
task, env, agent = make_stage("BlockAssemblyInsertSim", n, 22, task_kwargs={"grasp_states": states})
t0 = time.time()
for ep in range(epochs):
    agent.train_epoch()
    if (ep + 1) % every == 0 or ep == 0:
        torch.cuda.synchronize()
        aux = task.sim.INSERT_AUX.cpu().numpy()
        d, r = aux[:, 3], aux[:, 4]
        prog = task.sim.PROGRESS.cpu().numpy()
        print("epoch %5d  game reward %8.3f  len %6.1f  outcomes(succ, fail) %s  dist mm p10/p50/p90 %.1f/%.1f/%.1f  <20mm %.3f  rot p50 %.2f  <0.2 %.3f  both %.4f  lr %.2e"
              % (ep + 1, agent.game_rewards.get_mean()[0], agent.game_lengths.get_mean()[0], task.sim.TV_COUNT.cpu().tolist(),
                 *(np.quantile(d, [0.1, 0.5, 0.9]) * 1e3), float((d < 0.02).mean()), float(np.median(r)), float((r < 0.2).mean()),
                 float(((d < 0.02) & (r < 0.2)).mean()), agent.last_lr if hasattr(agent, "last_lr") else float("nan")), flush=True)
print(json.dumps({"wall_s": time.time() - t0, "grasp_states": task.grasp_states_source, "contact_stats": task.sim.CONTACT_STATS.cpu().tolist()}))
