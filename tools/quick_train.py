"""A few training epochs of a task with per-epoch timings (does it run, how fast).
usage: python tools/quick_train.py [num_envs] [epochs] [Task] [minibatch_size]"""
import sys, time
sys.path.insert(0,'.')
from seqdex_amd.stage import make_stage
n=int(sys.argv[1]) if len(sys.argv)>1 else 1024
task_name=sys.argv[3] if len(sys.argv)>3 else 'BlockAssemblyGraspSim'
t0=time.time()
task, env, agent = make_stage(task_name, n, 22, task_kwargs={'piles_per_type': 4}, minibatch_size=int(sys.argv[4]) if len(sys.argv)>4 else 0)
print('minibatch_size', agent.minibatch_size)
print('stage create s', time.time()-t0)
for ep in range(int(sys.argv[2]) if len(sys.argv)>2 else 4):
    r=agent.train_epoch()
    print('epoch',ep,'step %.4f play %.4f update %.4f total %.4f'%r[:4], 'a %.4f c %.4f kl %.5f lr %.2e'%(r[4][0],r[5][0],r[8][0],r[9]),
          'fps_step %.0f fps_total %.0f'%(n*8/r[0], n*8/r[3]), 'games', agent.game_rewards.get_mean(), agent.game_lengths.get_mean())
print('nc mean', task.sim.NCONTACTS.float().mean().item(), 'rew mean', task.rew_buf.mean().item())
