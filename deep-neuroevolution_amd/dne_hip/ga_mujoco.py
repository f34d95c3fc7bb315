"""es_distributed/ga.py (Deep GA) with MujocoPolicy, on the two engine kinds that run the policy: the pendulum ("env_id": "Pendulum-v0") and the
hard maze ("HardMaze-v0").  setup, run_master and run_worker have ga.py's signatures and are called directly, as ga_gpu.dense_ns_main is
(ga.setup keeps refusing the policy and points here).

An individual is a list of noise indices.  Its theta is the policy REINITIALISED on noise[seeds[0]] (ga.py:256-260: every weight column of the
three layers scaled to norm 1, every bias zero) plus noise_stdev * noise[seed] per further seed, in order (ga.py:262-263) -- csrc/mujoco_ga.h,
DESIGN.md section 16b.  The worker keeps the parents of the task's population in a bank on the device across tasks: a chain the bank holds is
kept, a chain that extends a banked one by one seed is made from it, and one promotion covers them; anything else is built from its genome.
Both routes give the same bits.  The children of a task -- a random parent's chain plus one fresh index -- go out in ONE dne_mujoco_ga_eval.

Decisions, where the reference leaves one:
  (a) ga.py:75-79 makes a fresh RunningStat(eps=1e-2) every iteration, so every GATask carries mean 0 and std 1; the increments of a batch are
      counted for ObCount and otherwise dropped.  Followed as written.
  (b) The worker's statistics branch unpacks policy.rollout's four values into three names (ga.py:25) and would raise.  Built as intended
      (SURVEY Q2): each child is flagged with probability calc_obstat_prob, the flagged episodes' sums come from the device, and the Result
      carries ob_sum, ob_sumsq and ob_count.
  (c) Action noise comes from the noise table through ac_off, chosen exactly as es.run_worker chooses it for this policy.
  (d) The evaluation episode is the elite's `params`, without action noise, under the environment's own step limit, reported apart.
  (e) WorkerClient's argument order is put right, as in ga.py here.
"""
import logging
import time

import numpy as np

from . import es
from .compat import GATask
from .dist import MasterClient, WorkerClient
from .es import Result, RunningStat, SharedNoiseTable, TaskPacer, collect_batch, flagged_ob_stats, log_generation, mujoco_engine_calls, parse_cutoff
from .ga import make_children, shard_children, truncate
from .policies import snapshot_extension

logger = logging.getLogger(__name__)


def setup(exp, engine=None, n_children=None, device_id=0):
    """ga.py:7-20 for MujocoPolicy: es.setup's engine (kind and shape from the experiment, the maze loaded), environment and policy, sized for
    n_children members an evaluation"""
    if exp['policy']['type'] != 'MujocoPolicy':
        raise NotImplementedError("ga_mujoco runs MujocoPolicy; {} runs under dne_hip.ga".format(exp['policy']['type']))
    n = max(n_children or exp['config']['episodes_per_batch'], 1)
    return es.setup(exp, engine=engine, n_pairs=(n + 1) // 2, device_id=device_id)


def genome_of(chain, noise_stdev):
    """a seed chain as the engine's genome (idx0, (idx1, power), ...): one power for every mutation"""
    chain = [int(s) for s in chain]
    return (chain[0], ) + tuple((s, float(noise_stdev)) for s in chain[1:])


def run_master(master_redis_cfg, log_dir, exp, *, engine=None, noise=None, max_iters=None):
    """ga.py:33-206"""
    from . import tabular_logger as tlogger
    logger.info('run_master: {}'.format(locals()))
    tlogger.start(log_dir)
    config, env, policy = setup(exp, engine=engine)
    engine = policy.engine
    master = MasterClient(master_redis_cfg)
    if not policy.get_trainable_flat().any():
        policy.initialize(0)                                          # the first task's params: the reference relies on TF's (unseeded) initialiser
    noise = noise if noise is not None else SharedNoiseTable()
    noise.attach(engine)
    tslimit, incr_tslimit_threshold, tslimit_incr_ratio, _, adaptive_tslimit = parse_cutoff(config.episode_cutoff_mode)
    episodes_so_far = timesteps_so_far = 0
    tstart = time.time()
    master.declare_experiment(exp)
    population, population_score = [], np.array([], np.float32)
    population_size, num_elites = exp['population_size'], exp['num_elites']
    it = 0
    while max_iters is None or it < max_iters:
        it += 1
        step_tstart = time.time()
        theta = policy.get_trainable_flat()
        assert theta.dtype == np.float32
        ob_stat = RunningStat(env.observation_space.shape, eps=1e-2)   # ga.py:75-79: a fresh one every iteration -- decision (a)
        curr_task_id = master.declare_task(GATask(params=theta, population=population, ob_mean=ob_stat.mean, ob_std=ob_stat.std,
                                                  timestep_limit=tslimit))
        tlogger.log('********** Iteration {} **********'.format(curr_task_id))
        batch = collect_batch(master, config, curr_task_id, check_pairs=False)
        episodes_so_far += batch.all_episodes
        timesteps_so_far += batch.all_timesteps
        curr_task_results, eval_rets = batch.results, batch.eval_rets
        ob_count_this_batch = 0
        for r in curr_task_results:                                   # ga.py:123-125: incremented, then dropped with the iteration
            if r.ob_count > 0:
                ob_stat.increment(r.ob_sum, r.ob_sumsq, r.ob_count)
                ob_count_this_batch += r.ob_count
        # ga.py:136-149: elites (old scores) + all children, keep the best population_size
        noise_inds_n = [list(c) for c in population[:num_elites]]
        returns_n2 = list(population_score[:num_elites])
        for r in curr_task_results:
            noise_inds_n.extend(list(c) for c in r.noise_inds_n)
            returns_n2.extend(r.returns_n2)
        returns_n2 = np.array(returns_n2, np.float32)
        lengths_n2 = np.concatenate([r.lengths_n2 for r in curr_task_results])
        population, population_score = truncate(engine, noise_inds_n, returns_n2, population_size)
        assert len(population) == population_size
        assert np.max(returns_n2) == population_score[0]
        logger.info('Elite: {} score: {}'.format(population[0], population_score[0]))
        policy.set_from_seeds(population[0], config.noise_stdev, noise)   # ga.py:151-158
        if adaptive_tslimit and (lengths_n2 == tslimit).mean() >= incr_tslimit_threshold:
            tslimit = int(tslimit_incr_ratio * tslimit)
        dt = time.time() - step_tstart
        log_generation(tlogger, [
            ("EpRewMax", returns_n2.max()), ("EpRewMean", returns_n2.mean()), ("EpLenMean", lengths_n2.mean()),
            ("EvalEpRewMean", np.mean(eval_rets) if eval_rets else np.nan), ("EvalEpCount", len(eval_rets)),
            ("EpisodesThisIter", lengths_n2.size), ("EpisodesSoFar", episodes_so_far),
            ("TimestepsThisIter", lengths_n2.sum()), ("TimestepsSoFar", timesteps_so_far), ("ObCount", ob_count_this_batch),
            ("TimeElapsedThisIter", dt), ("TimestepsPerSecondThisIter", lengths_n2.sum() / dt),
            ("TimeElapsed", time.time() - tstart)])
        if config.snapshot_freq != 0:
            import os.path as osp
            policy.save(osp.join(log_dir, ('snapshot_iter{:05d}_rew{}' + snapshot_extension()).format(
                curr_task_id, np.nan if not eval_rets else int(np.mean(eval_rets)))))
    return policy, population, population_score


def sync_bank(engine, bank, population, noise_stdev, reuse=True):
    """The engine's bank made to hold `population` (tuples of seeds), parent j = population[j]; `bank` is what it holds now.  With reuse, a
    chain the bank holds is kept, one that extends a banked chain by a seed is made from it, a one-seed chain is a root, and ONE promotion
    covers them; when a chain is none of these (or without reuse) every parent is built from its genome.  -> the new bank (a list)"""
    if not population or population == bank:
        return bank
    where = {}
    for j, c in enumerate(bank):
        where.setdefault(c, j)
    desc = []
    for c in population:
        if c in where:
            desc.append((where[c], -1, 0.0))
        elif len(c) > 1 and c[:-1] in where:
            desc.append((where[c[:-1]], c[-1], noise_stdev))
        elif len(c) == 1:
            desc.append((-1, c[0], 0.0))
        else:
            desc = None
            break
    if reuse and bank and desc is not None:
        parent, idx, power = zip(*desc)
        engine.mujoco_ga_promote(np.array(parent, np.int32), np.array(idx, np.int64), np.array(power, np.float32))
    else:
        engine.mujoco_ga_build([genome_of(c, noise_stdev) for c in population])
    return list(population)


def run_worker(master_redis_cfg, relay_redis_cfg, noise, *, min_task_runtime=.2, engine=None, max_tasks=None, seed=None,
               rank=0, world=1, reeval_after=1.0, bank_reuse=True):
    """ga.py:209-284 for one GPU: this worker's share of the episodes_per_batch children of a task in one device call, their parents in the
    engine's bank (bank_reuse False: rebuilt from their genomes every time the population changes).  As in es.run_worker the eval coin ADDS the
    evaluation episode (pushed first, as its own Result) to the task's children."""
    logger.info('run_worker: {}'.format(locals()))
    assert isinstance(noise, SharedNoiseTable)
    worker = WorkerClient(relay_redis_cfg, master_redis_cfg)         # decision (e)
    exp = worker.get_experiment()
    config, env, policy = setup(exp, engine=engine)
    engine = policy.engine
    noise.attach(engine)
    engine.mujoco_ga_reserve(max(int(exp['population_size']), 1))
    rs = np.random.RandomState(seed)
    worker_id = rs.randint(2 ** 31)
    assert policy.needs_ob_stat
    n = len(shard_children(max(config.episodes_per_batch, 1), rank, world))
    env_steps = env.max_episode_steps
    set_options, ob_stats = mujoco_engine_calls(engine, policy)
    pacer = TaskPacer(worker, max_tasks, reeval_after)
    bank = []
    while True:
        nxt = pacer.next_task()
        if nxt is None:
            break
        task_id, task_data = nxt
        assert isinstance(task_id, int) and isinstance(task_data, GATask)
        policy.set_ob_stat(task_data.ob_mean, task_data.ob_std)       # ga.py:224-225
        tslimit = task_data.timestep_limit
        tslimit = env_steps if tslimit is None else min(tslimit, env_steps)
        if rs.rand() < config.eval_prob:                              # ga.py:226-245 -- decision (d)
            policy.set_trainable_flat(task_data.params)
            engine.set_members(np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.float32))
            er, _, el = engine.eval_members(1, env_steps, rs.randint(0, 2 ** 32, size=1, dtype=np.uint64).astype(np.uint32))
            worker.push_result(task_id, Result(worker_id=worker_id, noise_inds_n=None, returns_n2=None, signreturns_n2=None,
                                               lengths_n2=None, eval_return=float(er[0]), eval_length=int(el[0]),
                                               ob_sum=None, ob_sumsq=None, ob_count=None))
        population = [tuple(int(s) for s in c) for c in task_data.population]
        bank = sync_bank(engine, bank, population, config.noise_stdev, reuse=bank_reuse)
        chains = make_children(population, n, noise, rs, policy.num_params)   # ga.py:251-254
        where = {}
        for j, c in enumerate(population):
            where.setdefault(c, j)
        parent = np.array([where[tuple(c[:-1])] if population else -1 for c in chains], np.int32)
        fresh = np.array([c[-1] for c in chains], np.int64)
        env_seeds = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
        # decisions (b) and (c): one coin a child, then where each episode's action noise starts in the table (es.run_worker's choice)
        flags = (rs.rand(n) < config.calc_obstat_prob) if config.calc_obstat_prob != 0 else np.zeros(n, bool)
        noisy = policy.ac_noise_std != 0
        ac_off = rs.randint(0, len(noise.noise) - env_steps * policy.num_actions + 1, size=n).astype(np.int64) if noisy else None
        set_options(n, policy.ac_noise_std if noisy else 0.0, ac_off, flags.astype(np.uint8))
        returns, signreturns, lengths = engine.mujoco_ga_eval(parent, fresh, np.full(n, config.noise_stdev, np.float32), tslimit, env_seeds)
        ob_sum, ob_sumsq, ob_count = flagged_ob_stats(ob_stats(n), flags) if flags.any() else (None, None, 0)
        worker.push_result(task_id, Result(
            worker_id=worker_id, noise_inds_n=[[int(s) for s in c] for c in chains], returns_n2=returns, signreturns_n2=signreturns,
            lengths_n2=lengths, eval_return=None, eval_length=None, ob_sum=ob_sum, ob_sumsq=ob_sumsq, ob_count=ob_count))
        pacer.pushed(task_id)
