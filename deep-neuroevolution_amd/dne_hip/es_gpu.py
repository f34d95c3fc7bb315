"""The ES loop of the reference's GPU tree (gpu_implementation/es.py) on the HIP engine: one process, no Redis -- TrainingState with
`snapshot.pkl` resume (es.py:40-83, 155-162, 278-283), antithetic offspring at a scheduled mutation power (es.py:175-187), the
adaptive episode cutoff (es.py:52-62, 273-276), the elite's test episodes before and after every update (es.py:190, 249) and the
reference's tabular keys (es.py:206-268).

Model: configurations/es_atari_config.json names `ModelVirtualBN` (models/batchnorm.py:52-123: conv 16 8x8/4, conv 32 4x4/2, fc 256 with
virtual batch norm from a reference batch).  The engine runs that architecture in one of two flat layouts, chosen by the optional config
key exp['flat_layout']:
  'es_distributed' (default)  the es_distributed parameterisation (DNE_KIND_ES, policies.py:319-330: conv / fc biases and a learnt BN scale
                              in the flat vector, 1 009 058 parameters at 18 actions); theta starts from policies.xavier_flat (SURVEY Q14:
                              the parity target is the CPU path).
  'native'                    ModelVirtualBN's own layout (DNE_KIND_ES_VBN, 1 008 450 parameters: no biases before the normalisation, no
                              BN scale, each BatchNorm/b a shift after it); theta starts as TrainingState.initialize does (es.py:73-75 ->
                              base.py:123-141): idx = noise.sample_index(rs, P), the first draw of the run's stream, then
                              theta = noise.get(idx, P) * scale_by (policies.vbn_scale_by) in fp32.
An engine passed in by the caller decides the layout by its kind.  The layout and P are recorded in snapshot.pkl; a resume under another
layout or P fails and names both (snapshots written before the key existed are 'es_distributed').  Not built: `load_from` (ga_legacy genomes).

es.py:144 takes exp['model'] from any of neuroevolution.models; `LargeModel` (models/dqn.py:39-47: conv 32/64/64, fc 512, 4 052 658 parameters at
18 actions, no batch norm) runs here too, on a DNE_KIND_GA_LARGE engine: theta is base slot 0, the pairs go through dne_es_eval (the streamed
fc shares a pair's theta and noise rows, csrc/forward_large.h: k_lfc_pair), there is no reference batch, and theta starts as
TrainingState.initialize does: idx = noise.sample_index(rs, P), the first draw, then noise.get(idx, P) * scale_by (ga_gpu.model_scale_by) in fp32.
flat_layout does not apply to it (only 'native', its one layout, is accepted).  The model's name is recorded in snapshot.pkl (a snapshot without
it is ModelVirtualBN); a resume under another model or P fails and names both.  A caller's engine of kind KIND_GA_LARGE selects this path.
Not built: every other model.  `Model` (dqn.py:24-36) is the network of DNE_KIND_GA, whose kernels take one member per group: dne_es_eval on
that kind is a tested refusal (tests/test_gpu_edges.py::test_refusals).  `ModelBN`, `SmallDQN` and the rest have no engine kind.

exp['game'] == 'maze' (gym_tensorflow.make's second environment, gym_tensorflow/maze/) with exp['model'] == 'SimpleClassifier' (models/simple.py:29-35)
runs on a DNE_KIND_MAZE engine: a whole 400-step episode per member inside one kernel (csrc/maze.h), no reference batch, no environment seeds (the
episode is deterministic; the seeds are still drawn, so the stream stays in step with the other kinds).  The maze file is exp['maze_file'], else hard_maze.txt
in the working directory (tf_maze.py:28), else the copy of the reference's file under tests/golden; theta starts as TrainingState.initialize does, noise.get(idx, 498) * policies.simple_scale_by() with
idx the stream's first draw; 'env_default' means 400 steps (tf_maze.py:32-33).  The game is recorded in snapshot.pkl (a snapshot without it is an Atari
run); a resume under another game fails and names both.  SimpleClassifier on an Atari game and the Atari models on the maze are refused.

exp['game'] == 'gym.CartPole-v1' (configurations/es_gym_config.json; gym_tensorflow.make sends every 'gym.*' name to GymEnv, a Python list of gym
environments stepped on the CPU) with exp['model'] == 'SimpleClassifier' runs on a DNE_KIND_CARTPOLE engine: a whole episode of at most 500 steps per
member inside one kernel (csrc/cartpole.h), no reference batch, every episode reset from its own environment seed of the run's stream (test
episodes included, as on Atari); theta starts as noise.get(idx, 386) * policies.simple_scale_by(KIND_CARTPOLE) with idx the stream's first draw;
'env_default' means 500 steps, and a larger cutoff (the shipped 5000) leaves gym's own 500 in force (GymEnv.reset ignores max_frames, tf_env.py:47-52).
A step is a frame.  The game is recorded in snapshot.pkl like the maze's.  Every other 'gym.*' name is refused by name: no other gym environment is built.

exp['model'] == 'LinearClassifier' (models/simple.py:23-27: one dense layer from the observation to the outputs) on game 'maze' or
'gym.CartPole-v1' runs on a DNE_KIND_DENSE engine with no hidden layer (csrc/dense.h: a dense stack of any small shape on the step environments,
whole episodes in k_dense_run) through the same episodic loop; theta starts as noise.get(idx, P) * policies.dense_scale_by(...) with idx the
stream's first draw.  A caller's engine of kind KIND_DENSE, of any shape, is accepted on its environment's game (its model is recorded as
'LinearClassifier' without hidden layers, else as dense_model_name writes the shape); one whose environment is not the game's is refused, naming
both.  SimpleClassifier keeps its own kinds and kernels.

exp['game'] == 'gym.Acrobot-v1' (csrc/acrobot.h) has no engine kind of its own: every run is a DNE_KIND_DENSE engine created on
the environment id ENV_ACROBOT, through the same episodic loop.  Without an engine exp['model'] == 'LinearClassifier' opens one with no hidden
layer (P = 21) and 'SimpleClassifier' one of hidden (16, 16), relu (P = 435); a caller's KIND_DENSE engine of any shape on that environment is
accepted (acrobot_run).  'env_default' means 500 steps and a larger cutoff leaves 500 in force, as on the cart-pole; the game is recorded in
snapshot.pkl.  'gym.MountainCar-v0', 'gym.CartPole-v0', 'gym.Acrobot-v0' and every other 'gym.*' name stay refused by name.

Where the arithmetic lives: ranks, sum_i w_i * noise[idx_i] / 2N, -g + l2coeff * theta and the optimizer step are dne_es_update on the device
(the same formulas as es_distributed: es.py:227-246 here = es_distributed/es.py:281-301).  The GPU tree's SGD keeps v = momentum * v + g
(neuroevolution/optimizers.py:49-51) where es_distributed keeps (1 - momentum) * g: with u = (1 - momentum) * v that is the engine's SGD at
stepsize / (1 - momentum) -- equal in real arithmetic, not bit for bit; Adam is the same formula in both trees.
Unseeded streams of the reference (np.random.RandomState() at es.py:151, the environments' seeds) are seeded here.
"""
import os
import pickle
import time

import numpy as np

from . import _lib
from .es import SharedNoiseTable, get_ref_batch, optimizer_args, parse_cutoff
from .ga_gpu import Offspring, Schedule, model_scale_by
from . import acrobot_run, cartpole_run
from .acrobot_run import ACROBOT_GAME
from .cartpole_run import CARTPOLE_GAME
from .maze_run import MAZE_FILE, MAZE_MODEL, attach_table, check_engine, maze_file, open_engine   # noqa: F401 (MAZE_FILE, maze_file: read as es_gpu's by callers)

# exp['model'] (es.py:144): neuroevolution/models/batchnorm.py:52 (in either flat layout, FLAT_LAYOUTS) and models/dqn.py:39
MODEL_KINDS = {'ModelVirtualBN': _lib.KIND_ES, 'LargeModel': _lib.KIND_GA_LARGE}
FLAT_LAYOUTS = {'es_distributed': _lib.KIND_ES, 'native': _lib.KIND_ES_VBN}   # exp['flat_layout'] -> the engine kind that runs it
LINEAR_MODEL = 'LinearClassifier'        # neuroevolution/models/simple.py:23-27, on a KIND_DENSE engine without hidden layers
DENSE_GAMES = {_lib.KIND_MAZE: 'maze', _lib.KIND_CARTPOLE: CARTPOLE_GAME, _lib.KIND_PENDULUM: 'Pendulum-v0',
               _lib.ENV_ACROBOT: ACROBOT_GAME}   # a KIND_DENSE engine's environment -> its game


def dense_model_name(engine):
    """the model a KIND_DENSE engine runs, as snapshot.pkl records it"""
    if not engine.hidden:
        return LINEAR_MODEL
    return 'Dense({}; {})'.format(', '.join(str(w) for w in engine.hidden), 'relu' if engine.nonlin == _lib.DENSE_NONLINS['relu'] else 'tanh')


class TrainingState(object):
    """What snapshot.pkl holds (es.py:40-83): the counters, the episode cutoff with its growth rule, the mutation-power schedule, theta and
    the optimizer's state -- here as plain arrays fetched from / pushed to the device around a pickle."""
    COUNTERS = ('num_frames', 'timesteps_so_far', 'time_elapsed', 'validation_timesteps_so_far', 'it')

    def __init__(self, exp):
        for name in self.COUNTERS:
            setattr(self, name, 0)
        self.mutation_power = Schedule.from_config(exp['mutation_power'])
        limit, grow_at, grow_by, limit_max, adaptive = parse_cutoff(exp['episode_cutoff_mode'])
        self.tslimit, self.adaptive_tslimit = limit, adaptive
        self.incr_tslimit_threshold, self.tslimit_incr_ratio = grow_at, grow_by
        if adaptive:
            self.tslimit_max = limit_max
        self.flat_layout = 'es_distributed'   # FLAT_LAYOUTS key of the run (main sets it); a snapshot without it predates the choice
        self.game = None                      # exp['game'] of a maze or cart-pole run ('maze', 'gym.CartPole-v1'); None: an Atari game (a snapshot without it predates the maze)
        self.model = 'ModelVirtualBN'         # MODEL_KINDS key of the run (main sets it); a snapshot without it predates LargeModel
        self.num_params = None
        self.theta = None
        self.optimizer = None          # (m, v, t) of the device optimizer, None before the first update
        self.stream = None             # the index / environment-seed stream's position (an extension: the reference's stream is unseeded,
                                       # es.py:151; with it a resumed run continues exactly where an uninterrupted one would be)

    def sample(self, schedule):
        return schedule.value(iteration=self.it, timesteps_so_far=self.timesteps_so_far)

    def pull(self, engine):
        self.theta = engine.get_theta()
        self.optimizer = engine.optimizer_get_state()

    def push(self, engine):
        engine.set_theta(self.theta)
        engine.optimizer_reset()
        if self.optimizer is not None and self.optimizer[2] > 0:
            engine.optimizer_set_state(*self.optimizer)


def engine_optimizer(opt):
    """(kind, stepsize, beta1-or-momentum, beta2, epsilon) for dne_es_update; the GPU tree's SGD mapped as the module docstring says"""
    step, first, beta2, eps = optimizer_args(opt)
    if opt['type'] == 'sgd':
        if first >= 1.0:
            raise ValueError("sgd momentum {!r}: the engine's SGD runs at stepsize / (1 - momentum), momentum must be below 1".format(first))
        step = step / (1.0 - first)
    return opt['type'], step, first, beta2, eps


def _env_limit(engine):
    """the environment's own episode bound: env_default_timestep_cutoff of the maze (tf_maze.py:32-33), CartPole-v1's 500, gym's TimeLimit for Atari"""
    kind = getattr(engine, 'env_kind', engine.kind)   # (a KIND_DENSE engine: the environment it was created on)
    if kind == _lib.KIND_CARTPOLE:
        return _lib.CARTPOLE_STEPS
    if kind == _lib.ENV_ACROBOT:
        return _lib.ACROBOT_STEPS
    return _lib.MAZE_STEPS if kind == _lib.KIND_MAZE else _lib.ENV_MAX_EPISODE_STEPS


def _episodes_of_theta(engine, n, tslimit, rs):
    """n episodes of the unperturbed theta (monitor_eval_repeated([(theta, 0)], ...), es.py:190, 249): pairs at mutation power 0 --
    theta + 0 * eps twice, every episode under its own environment seed"""
    limit = _env_limit(engine) if tslimit is None else min(int(tslimit), _env_limit(engine))
    rets, lens = [], []
    left = int(n)
    while left > 0:
        pairs = min((left + 1) // 2, engine.max_members // 2)
        seeds = rs.randint(0, 2 ** 32, size=2 * pairs, dtype=np.uint64).astype(np.uint32)
        r, _, l = engine.es_eval(np.zeros(pairs, np.int64), 0.0, limit, seeds)
        rets.append(np.asarray(r).reshape(-1)); lens.append(np.asarray(l).reshape(-1))
        left -= 2 * pairs
    return np.concatenate(rets)[:n], np.concatenate(lens)[:n]


def main(log_dir, engine=None, noise=None, seed=0, max_iters=None, ref_count=128, **exp):
    """gpu_implementation/es.py:139-288.  Returns the TrainingState (theta and optimizer state pulled from the device)."""
    from . import policies, tabular_logger as tlogger
    tlogger.start(log_dir)
    if 'load_from' in exp:
        raise NotImplementedError("load_from (es.py:164-171: a ga_legacy genome as the first theta) is not built")
    n_pairs = exp['population_size'] // 2
    asked = exp['model'] if engine is None else exp.get('model')   # the caller's engine decides; a name given with it must agree
    game = exp.get('game')
    if isinstance(game, str) and game.startswith('gym.') and game not in (CARTPOLE_GAME, ACROBOT_GAME):
        raise NotImplementedError("game {!r}: of gym_tensorflow's 'gym.*' environments this loop runs {!r} only, and {!r} on a dense policy".format(
            game, CARTPOLE_GAME, ACROBOT_GAME))
    if game == ACROBOT_GAME:                                          # no kind of its own: a KIND_DENSE engine on ENV_ACROBOT, the caller's or one of the two named shapes
        acrobot_run.check_engine(engine)
        if engine is None and asked not in acrobot_run.MODEL_HIDDEN:
            raise NotImplementedError("model {!r} on game {!r}: without an engine this loop runs {!r} and {!r} there".format(
                asked, game, LINEAR_MODEL, MAZE_MODEL))
    acro = game == ACROBOT_GAME
    dense = engine.kind == _lib.KIND_DENSE if engine is not None else (asked == LINEAR_MODEL or acro)   # a dense stack on a step environment (csrc/dense.h)
    cart = game == CARTPOLE_GAME or (engine is not None and engine.kind == _lib.KIND_CARTPOLE)
    maze = not cart and (game == 'maze' or (engine is not None and engine.kind == _lib.KIND_MAZE))
    if dense:
        if engine is None and not (cart or maze or acro):
            raise NotImplementedError("model {!r} on game {!r}: this loop runs it on 'maze' and {!r}, and on {!r}".format(asked, game, CARTPOLE_GAME, ACROBOT_GAME))
        if engine is not None:
            if DENSE_GAMES.get(engine.env_kind) != game:
                raise ValueError("game {!r} asked for, the engine passed in (kind {} on environment kind {}) runs {!r}".format(
                    game, engine.kind, engine.env_kind, DENSE_GAMES.get(engine.env_kind)))
            if engine.env_kind == _lib.KIND_PENDULUM:
                raise NotImplementedError("game {!r}: this loop runs a KIND_DENSE engine on 'maze' and {!r}".format(game, CARTPOLE_GAME))
        if asked is not None and engine is not None and asked != (acrobot_run.simple_name(engine, asked) or dense_model_name(engine)):
            raise ValueError("model {!r} asked for, the engine passed in (kind {}) runs {!r}".format(asked, engine.kind, dense_model_name(engine)))
    elif cart:                                                        # gym_tensorflow.make(game='gym.CartPole-v1'): GymEnv's cart-pole under SimpleClassifier
        if game != CARTPOLE_GAME:
            raise ValueError("game {!r} asked for, the engine passed in (kind {}) runs {!r}".format(game, engine.kind, CARTPOLE_GAME))
        cartpole_run.check_engine(engine)
        if asked is not None and asked != MAZE_MODEL:
            raise NotImplementedError("model {!r} on game {!r}: this loop runs {!r} there".format(asked, CARTPOLE_GAME, MAZE_MODEL))
    elif maze:                                                        # gym_tensorflow.make(game='maze'): the hard maze under SimpleClassifier
        if exp.get('game') != 'maze':
            raise ValueError("game {!r} asked for, the engine passed in (kind {}) runs 'maze'".format(exp.get('game'), engine.kind))
        check_engine(engine)
        if asked is not None and asked != MAZE_MODEL:
            raise NotImplementedError("model {!r} on game 'maze': this loop runs {!r} there".format(asked, MAZE_MODEL))
    elif asked == MAZE_MODEL:
        raise NotImplementedError("model {!r} on game {!r}: it runs on game 'maze' only".format(asked, exp.get('game')))
    episodic = maze or cart or acro                                 # a whole episode per member in one kernel: one layout, no reference batch, no frame skip
    if not episodic and asked is not None and asked not in MODEL_KINDS:
        raise NotImplementedError("model {!r}: this loop runs {}".format(asked, sorted(MODEL_KINDS)))
    large = not episodic and (engine.kind if engine is not None else MODEL_KINDS[asked]) == _lib.KIND_GA_LARGE
    model = (asked if engine is None else acrobot_run.simple_name(engine, asked) or dense_model_name(engine)) if dense else MAZE_MODEL if episodic else 'LargeModel' if large else 'ModelVirtualBN'
    if asked is not None and asked != model:
        raise ValueError("model {!r} asked for, the engine passed in (kind {}) runs {!r}".format(asked, engine.kind, model))
    if episodic:                                                    # one flat layout, no reference batch; the maze: the walls instead
        layout = 'native'
        if exp.get('flat_layout', layout) != layout:
            raise ValueError("flat_layout {!r}: {} has one layout, 'native'".format(exp['flat_layout'], model))
        if dense:
            if acro:
                engine, noise = acrobot_run.open_engine(engine, noise, 2 * n_pairs, asked)
            else:
                if engine is None:
                    engine = _lib.Engine(_lib.KIND_DENSE, 2, max_members=2 * n_pairs, env=_lib.KIND_MAZE if maze else _lib.KIND_CARTPOLE, hidden=(), nonlin='relu')
                if maze:
                    engine.maze_set_walls(*_lib.load_maze(maze_file(exp)))
                noise = attach_table(engine, noise)
            scale_by = policies.dense_scale_by(engine.env_kind, engine.hidden, engine.n_actions)
        elif maze:
            engine, noise = open_engine(exp, engine, noise, 2 * n_pairs)
        else:
            engine, noise = cartpole_run.open_engine(engine, noise, 2 * n_pairs)
        if not dense:
            scale_by = policies.simple_scale_by(engine.kind)
    elif large:                                                       # one flat layout, the model's own; no reference batch
        layout = 'native'
        if exp.get('flat_layout', layout) != layout:
            raise ValueError("flat_layout {!r}: LargeModel has one layout, 'native'".format(exp['flat_layout']))
        if engine is None:
            engine = _lib.Engine(_lib.KIND_GA_LARGE, 18, max_members=2 * n_pairs)
        scale_by = model_scale_by(engine.n_actions, _lib.KIND_GA_LARGE)
        engine.ga_set_init_scale(scale_by)
    elif engine is None:
        layout = exp.get('flat_layout', 'es_distributed')
        if layout not in FLAT_LAYOUTS:
            raise ValueError("flat_layout {!r}: expected one of {}".format(layout, sorted(FLAT_LAYOUTS)))
        engine = _lib.Engine(FLAT_LAYOUTS[layout], 18, max_members=2 * n_pairs, ref_count=ref_count)
    else:                                                           # the caller's engine decides
        layout = {k: name for name, k in FLAT_LAYOUTS.items()}.get(engine.kind)
        if layout is None or exp.get('flat_layout', layout) != layout:
            raise ValueError("flat_layout {!r} asked for, the engine passed in (kind {}) runs {!r}".format(
                exp.get('flat_layout'), engine.kind, layout))
    if not episodic:                                                # (open_engine attached the maze's and the cart-pole's)
        noise = noise if noise is not None else SharedNoiseTable()
        noise.attach(engine)
    rs = np.random.RandomState(seed)
    all_tstart = tstart = time.time()
    try:                                                            # es.py:155-162: resume
        with open(os.path.join(log_dir, 'snapshot.pkl'), 'rb') as file:
            state = pickle.load(file)
        tlogger.log("Loaded iteration {} from {}".format(state.it, log_dir))
        was_game = getattr(state, 'game', None)
        if was_game != ('maze' if maze else CARTPOLE_GAME if cart else ACROBOT_GAME if acro else None):
            raise ValueError("snapshot.pkl in {} holds game {!r}; this run is game {!r}".format(
                log_dir, was_game if was_game is not None else 'an Atari game', exp.get('game')))
        was_model = getattr(state, 'model', 'ModelVirtualBN')
        if was_model != model or ((large or episodic) and int(np.asarray(state.theta).size) != engine.P):
            raise ValueError("snapshot.pkl in {} holds model {!r} with P = {}; this run is model {!r} with P = {}".format(
                log_dir, was_model, int(np.asarray(state.theta).size), model, engine.P))
        was = (getattr(state, 'flat_layout', 'es_distributed'), int(np.asarray(state.theta).size))
        if not large and not episodic and was != (layout, engine.P):
            raise ValueError("snapshot.pkl in {} holds flat_layout {!r} with P = {}; this run is flat_layout {!r} with P = {}".format(
                log_dir, was[0], was[1], layout, engine.P))
    except FileNotFoundError:
        state = TrainingState(exp)
        if episodic or large or layout == 'native':                             # es.py:173 -> es.py:73-75 -> model.randomize(rs, noise), base.py:123-141
            idx = noise.sample_index(rs, engine.P)
            state.theta = noise.get(idx, engine.P) * (scale_by if large or episodic else policies.vbn_scale_by(engine.n_actions))
        else:
            state.theta = policies.xavier_flat(engine.n_actions, seed)   # es.py:173: state.initialize(rs, noise, worker.model)
    state.flat_layout, state.num_params, state.model = layout, engine.P, model
    state.game = 'maze' if maze else CARTPOLE_GAME if cart else ACROBOT_GAME if acro else None
    state.push(engine)
    if not large and not episodic:                                               # ModelVirtualBN.requires_ref_batch (batchnorm.py:60-62); LargeModel has none
        env = policies.HipAtariEnv(engine, seed=seed)
        ref = np.stack(get_ref_batch(env, batch_size=engine.ref_count, random_stream=np.random.RandomState(seed)))
        engine.set_ref_batch(np.rint(ref * 255.0).astype(np.uint8))
    opt = engine_optimizer(exp['optimizer'])
    initial_performance, _ = _episodes_of_theta(engine, exp['num_test_episodes'], None, rs)   # es.py:190
    if getattr(state, 'stream', None) is not None:
        rs.set_state(state.stream)
    iters = 0
    while max_iters is None or iters < max_iters:
        iters += 1
        tstart_iteration = time.time()
        if state.timesteps_so_far >= exp['timesteps']:
            break
        # es.py:175-187: population_size // 2 indices, each evaluated at +power and -power; 5000 frames = tslimit * 4 (es.py:198)
        power = state.sample(state.mutation_power)
        idx = np.array([noise.sample_index(rs, engine.P) for _ in range(n_pairs)], np.int64)
        seeds = rs.randint(0, 2 ** 32, size=2 * n_pairs, dtype=np.uint64).astype(np.uint32)
        limit = _env_limit(engine) if state.tslimit is None else min(int(state.tslimit), _env_limit(engine))
        rets, sgn, lens = engine.es_eval(idx, power, limit, seeds)
        results = [Offspring(int(i), [float(r[0]), float(r[1])], [int(l[0]), int(l[1])]) for i, r, l in zip(idx, rets, lens)]
        state.num_frames += int(np.sum(lens)) * (1 if episodic else 4)              # (the maze and the cart-pole have no frame skip: a step is a frame)
        state.it += 1
        rewards = np.array([b for a in results for b in a.rewards])
        timesteps_this_iter = int(sum(a.training_steps for a in results))
        state.timesteps_so_far += timesteps_this_iter
        if exp['return_proc_mode'] != 'centered_rank':
            raise NotImplementedError(exp['return_proc_mode'])      # es.py:231-234
        # es.py:227-246 on the device: centered ranks of the 2N returns, g = sum_i (r+ - r-) noise[idx_i] / 2N, step on -g + l2coeff * theta
        update_ratio = engine.es_update(idx, rets, sgn, 'centered_rank', opt[0], exp['l2coeff'], *opt[1:])
        time_elapsed_this_iter = time.time() - tstart_iteration
        state.time_elapsed += time_elapsed_this_iter
        test_evals, test_lens = _episodes_of_theta(engine, exp['num_test_episodes'], None, rs)   # es.py:249
        dt = time.time() - tstart_iteration
        for key, val in (('Iteration', state.it), ('MutationPower', power), ('TimestepLimitPerEpisode', state.tslimit),
                         ('PopulationEpRewMax', np.max(rewards)), ('PopulationEpRewMean', np.mean(rewards)),
                         ('PopulationEpRewMedian', np.median(rewards)), ('PopulationEpCount', len(rewards)),
                         ('PopulationTimesteps', timesteps_this_iter), ('UpdateRatio', float(update_ratio)),
                         ('TestRewMean', np.mean(test_evals)), ('TestRewMedian', np.median(test_evals)), ('TestEpCount', len(test_evals)),
                         ('TestEpLenSum', int(np.sum(test_lens))), ('InitialRewMax', np.max(initial_performance)),
                         ('InitialRewMean', np.mean(initial_performance)), ('InitialRewMedian', np.median(initial_performance)),
                         ('TimestepsThisIter', timesteps_this_iter), ('TimestepsPerSecondThisIter', timesteps_this_iter / dt),
                         ('TimestepsComputed', state.num_frames), ('TimestepsSoFar', state.timesteps_so_far),
                         ('TimeElapsedThisIter', time_elapsed_this_iter), ('TimeElapsedThisIterTotal', dt),
                         ('TimeElapsed', state.time_elapsed), ('TimeElapsedTotal', time.time() - all_tstart)):
            tlogger.record_tabular(key, val)
        tlogger.dump_tabular()
        fps = state.timesteps_so_far / (time.time() - tstart)
        tlogger.log('Timesteps Per Second: {:.0f}. Elapsed: {:.2f}h'.format(fps, (time.time() - all_tstart) / 3600))
        if state.adaptive_tslimit:                                  # es.py:273-276 (a pair's two lengths summed against the limit, as written there)
            if np.mean([a.training_steps >= state.tslimit for a in results]) > state.incr_tslimit_threshold:
                state.tslimit = min(state.tslimit * state.tslimit_incr_ratio, state.tslimit_max)
                tlogger.log('Increased threshold to {}'.format(state.tslimit))
        state.pull(engine)                                          # es.py:278-283
        state.stream = rs.get_state()
        os.makedirs(log_dir, exist_ok=True)
        with open(os.path.join(log_dir, 'snapshot.pkl'), 'wb') as file:
            pickle.dump(state, file)
        if state.timesteps_so_far >= exp['timesteps']:
            break
    state.pull(engine)
    return state
