"""Exploration for the chain on learned policies: stage 0 (insert policy + transition value), statistics of that transition value over random
orientations, then BlockAssemblyOrient trained with minibatches of 2048 under gate `gate`: piles harvested per brick-type group.
usage: python tools/orient_probe.py N insert_epochs orient_epochs gate"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from seqdex_amd.scripts.chain_training import prepare_tvalue_and_insert_policy, tvalue_over_random_orientations  # noqa: E402
from seqdex_amd.stage import make_stage  # noqa: E402

n, ie, oe, gate = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4])
tv, _, ist = prepare_tvalue_and_insert_policy(n, ie, seed=22)
print("stage 0:", json.dumps(ist), flush=True)
print("T over 200 000 random orientations:", json.dumps(tvalue_over_random_orientations(tv)), flush=True)
task, env, agent = make_stage("BlockAssemblyOrient", n, 22, task_kwargs={"tvalue_gate": gate, "piles_per_type": 64}, minibatch_size=2048)
task.sim.set_tvalue_weights(tv)
t0 = time.time()
for ep in range(oe):
    agent.train_epoch()
    if (ep + 1) % 100 == 0 or ep == 0:
        torch.cuda.synchronize()
        print("epoch %4d  game reward %8.3f  len %5.1f  piles harvested/type %s  T-value outcomes %s  tvalue mean %.4f  %.0f env-steps/s"
              % (ep + 1, agent.game_rewards.get_mean()[0], agent.game_lengths.get_mean()[0], task.sim.PILE_HARVEST_COUNT.cpu().tolist(), task.sim.TV_COUNT.cpu().tolist(),
                 float(task.sim.TVALUE.mean()), n * 8 * (ep + 1) / (time.time() - t0)), flush=True)
