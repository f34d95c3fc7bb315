"""NS-ES and NSR-ES on the hard maze: the meta-population loop of es_distributed/nses.py:58-316 as ONE process on a DNE_KIND_MAZE engine, with
the conventions of es_gpu.py (seeded streams, `snapshot.pkl` resume, tabular keys, Schedule; the engine through maze_run.open_engine).

The maze is the reference's deceptive domain: the behaviour characterisation (BC) of a policy is where its navigator ended, MazeFinalState
(gym_tensorflow/maze/tf_maze.py:64-66), one float32 point (x, y).  Novelty is nses.py:12-32 on such points -- the mean distance to the k
nearest archive points -- scored on the device by k_maze_novelty (csrc/maze_novelty.h): the 2N final positions of a
generation are read where k_maze_rollout left them, the archive lives on the device, and only the 2N novelties come back.

Configuration (the rest as es_gpu.main: population_size, mutation_power, episode_cutoff_mode, l2coeff, optimizer, timesteps, maze_file):
  exp['game'] == 'maze' and exp['model'] == 'SimpleClassifier'; anything else is refused, naming both
  exp['algo_type']          'ns' (novelty alone) or 'nsr' (novelty ranks averaged with reward ranks, nses.py:226-228)
  exp['novelty_search']     {k, population_size: M, num_rollouts: 1, selection_method} as configurations/frostbite_nsres.json; num_rollouts
                            other than 1 is refused (the maze is deterministic: every rollout of a theta ends at the same point); a selection
                            method other than 'round_robin' and 'novelty_prob' raises NotImplementedError, as nses.py:305-306 does
  exp['return_proc_mode']   the three modes of nses.py:217-228, applied by nses.blend_and_update with the novelty in the aux slot

Initial state: the M thetas start as TrainingState.initialize does, each with its own draw -- idx = noise.sample_index(rs, 498), theta =
noise.get(idx, 498) * policies.simple_scale_by(), for m = 0 .. M-1 in order -- with a zeroed optimizer state; each is evaluated once at
power 0 and its final (x, y) is appended to the archive (nses.py:95-117).

One iteration for parent p: theta and optimizer state in place; the power; population_size // 2 indices and the environment seeds (the maze
reads no seed; they are drawn so that the stream stays in step with the other drivers); es_eval; engine.maze_novelty(k) over the 2N members;
nses.blend_and_update; one episode of the updated theta at power 0, whose return and length are logged and whose final (x, y) is appended
to the archive device to device (nses.py:246-247); theta and optimizer state stored back.

Two decisions of this driver, where the reference never meets the case:
  * a non-finite novelty becomes 0.0 before any rank.  A NaN position (a policy whose outputs went NaN) has NaN novelty, and argsort would
    rank that NaN above every number: the least informative member would pull the update hardest.  0.0 is the lowest novelty there is.
  * 'novelty_prob' with novelties whose sum is 0 or not finite selects uniformly; nses.py:301 would divide by that sum.
'novelty_prob' evaluates all M thetas in ONE evaluation of M members (base slots 1 .. M at scale 0) and scores them in one maze_novelty call.

snapshot.pkl holds the thetas, optimizer states, archive, current parent, counters, the stream and algo = 'nses'; a resume pushes the
archive back to the device.  A resume from a snapshot of es_gpu.main, or under another algo_type, M or k, raises and names both.

A dense policy of any small shape (DNE_KIND_DENSE, csrc/dense.h) runs the same loop with novelty over final states (csrc/dense_novelty.h,
DESIGN.md section 17b): a caller's engine of kind KIND_DENSE on its environment's game ('maze' or 'gym.CartPole-v1'; the pendulum is not built;
another game, or a model name that is not es_gpu.dense_model_name(engine), is a ValueError naming both), or no engine and exp['model'] ==
'LinearClassifier' on one of the two games, which opens a KIND_DENSE engine with no hidden layer.  Every other combination takes the path
above and says what it always said.  What differs sits behind _MazeSide / _DenseSide: P, the initial scale (policies.dense_scale_by of the
shape), the archive and novelty calls (dense_archive_*, dense_novelty: a BC is D floats of the final state record -- the maze's (x, y), the
cart-pole's (x, x_dot, theta, theta_dot)), the step limit and the engine opener.  The stream is the maze driver's draw for draw, so a (16, 16)
relu dense engine on the maze writes the rows, thetas and archive of the SimpleClassifier run.  On the cart-pole num_rollouts = R >= 1 is
nses.py:34-39's get_mean_bc: R episodes of theta at power 0 under R fresh seeds, the archive point the float64 mean of their BCs cast to
float32, appended from the host (R = 1: device to device); the logged test return is the first episode's.  snapshot.pkl records game, model,
num_params and, on a dense run, num_rollouts (the maze path runs 1 and its snapshot keeps the attributes it had); a resume under another of
them raises and names both sides.
'gym.Acrobot-v1' (csrc/acrobot.h) runs here as the cart-pole does -- seeds, num_rollouts >= 1, own limit 500 -- with the BC
(theta1, theta2, omega1, omega2) of the final state, D = 4: a caller's KIND_DENSE engine created on ENV_ACROBOT, or no engine and exp['model'] ==
'LinearClassifier' or 'SimpleClassifier' (hidden (16, 16), relu), opened by acrobot_run.
"""
import os
import pickle
import time

import numpy as np

from . import _lib, nses
from .es import pack_records, parse_cutoff
from . import acrobot_run
from .es_gpu import ACROBOT_GAME, CARTPOLE_GAME, DENSE_GAMES, LINEAR_MODEL, _env_limit, _episodes_of_theta, dense_model_name
from .ga_gpu import Schedule
from .maze_run import MAZE_MODEL, attach_table, check_engine, maze_file, open_engine, step_limit

ALGO = 'nses'
ALGO_TYPES = ('ns', 'nsr')
SELECTION_METHODS = ('round_robin', 'novelty_prob')
PROC_MODES = ('centered_rank', 'sign', 'centered_sign_rank')


class NsesState(object):
    """What snapshot.pkl holds, and what main returns."""

    def __init__(self, exp, pop_size, k):
        self.algo, self.algo_type, self.pop_size, self.k = ALGO, exp['algo_type'], pop_size, k
        self.game, self.model, self.num_params = 'maze', MAZE_MODEL, None   # (main sets them; a dense run adds num_rollouts, a maze run has 1)
        self.it = self.timesteps_so_far = self.num_frames = 0
        self.time_elapsed = 0.0
        self.mutation_power = Schedule.from_config(exp['mutation_power'])
        self.tslimit, self.incr_tslimit_threshold, self.tslimit_incr_ratio, self.tslimit_max, self.adaptive_tslimit = \
            parse_cutoff(exp['episode_cutoff_mode'])
        self.thetas, self.optimizers = [], []      # per parent: theta [P]; (m, v, t) of the device optimizer
        self.archive = np.zeros((0, 2), np.float32)   # the BCs in insertion order, [size][D]
        self.curr_parent = 0
        self.parents = []                          # the parent of every iteration so far
        self.novelty_log = []                      # (NoveltyMean, NoveltyMax) of every iteration so far
        self.stream = None


def sanitized(novelty):
    """float64 novelties with every non-finite one at 0.0 (the module docstring says why)"""
    novelty = np.asarray(novelty, np.float64)
    return np.where(np.isfinite(novelty), novelty, 0.0)


def _push_parent(engine, theta, optimizer):
    engine.set_theta(theta)
    engine.optimizer_reset()
    if optimizer[2] > 0:
        engine.optimizer_set_state(*optimizer)


def select_parent(engine, state, method, k, limit, rs, novelty=None):
    """nses.py:293-306; novelty(k, n=M): the scoring call of the run's side (None: the maze's)"""
    M = state.pop_size
    if method == 'round_robin':
        return (state.curr_parent + 1) % M
    for m in range(M):
        engine.set_theta(state.thetas[m], slot=m + 1)
    engine.set_members(np.arange(1, M + 1, dtype=np.int32), np.zeros(M, np.int64), np.zeros(M, np.float32))
    seeds = rs.randint(0, 2 ** 32, size=M, dtype=np.uint64).astype(np.uint32)
    engine.eval_members(M, limit, seeds)
    nov = np.asarray((novelty or engine.maze_novelty)(k, n=M), np.float64)
    total = float(np.sum(nov))
    probs = nov / total if np.isfinite(total) and total > 0.0 and np.all(np.isfinite(nov)) else np.full(M, 1.0 / M)
    return int(rs.choice(range(M), 1, p=probs)[0])


class _MazeSide(object):
    """what the loop asks of a DNE_KIND_MAZE engine under SimpleClassifier: P = 498, final (x, y) points, k_maze_novelty"""
    game, model = 'maze', MAZE_MODEL

    def __init__(self, exp, engine, noise, max_members):
        from . import policies
        self.engine, self.noise = open_engine(exp, engine, noise, max_members)
        self.scale_by = policies.simple_scale_by()
        self.archive_clear, self.archive_append, self.archive = self.engine.maze_archive_clear, self.engine.maze_archive_append, self.engine.maze_archive
        self.novelty = self.engine.maze_novelty

    def step_limit(self, tslimit):
        return step_limit(tslimit)

    def episodes_to_archive(self, rollouts, tslimit, rs):
        """one episode of the engine's theta at power 0, its final position appended device to device -> (returns, lengths)"""
        out = _episodes_of_theta(self.engine, 1, tslimit, rs)
        self.archive_append(n=1)
        return out


class _DenseSide(object):
    """the same of a DNE_KIND_DENSE engine on the maze, the cart-pole or the acrobot: P and the scale of its shape, BCs of D floats, k_dense_novelty"""

    def __init__(self, exp, engine, noise, max_members):
        from . import policies
        self.game = exp.get('game')
        made = engine is None
        if made and self.game == ACROBOT_GAME:
            engine = acrobot_run.make_engine(max_members, exp.get('model'))
        elif made:
            engine = _lib.Engine(_lib.KIND_DENSE, 2, max_members=max_members, env=_lib.KIND_MAZE if self.game == 'maze' else _lib.KIND_CARTPOLE,
                                 hidden=(), nonlin='relu')
        self.model = (acrobot_run.simple_name(engine, exp.get('model')) if acrobot_run.is_engine(engine) else None) or dense_model_name(engine)
        if engine.env_kind == _lib.KIND_MAZE:
            engine.maze_set_walls(*_lib.load_maze(maze_file(exp)))
        self.engine, self.noise = engine, attach_table(engine, noise)
        self.scale_by = policies.dense_scale_by(engine.env_kind, engine.hidden, engine.n_actions)
        self.archive_clear, self.archive_append, self.archive = engine.dense_archive_clear, engine.dense_archive_append, engine.dense_archive
        self.novelty = engine.dense_novelty

    def step_limit(self, tslimit):
        return _env_limit(self.engine) if tslimit is None else min(int(tslimit), _env_limit(self.engine))

    def episodes_to_archive(self, rollouts, tslimit, rs):
        """nses.py:34-39 get_mean_bc: `rollouts` episodes of the engine's theta at power 0 under fresh seeds; the archive point is their BCs'
        float64 mean cast to float32, from the host -- one episode: its BC, device to device -> (returns, lengths)"""
        if rollouts == 1:
            out = _episodes_of_theta(self.engine, 1, tslimit, rs)
            self.archive_append(n=1)
            return out
        rets, lens, bcs = [], [], []
        left, most = int(rollouts), 2 * (self.engine.max_members // 2)   # (_episodes_of_theta's own evaluations: each call below is one of them)
        while left > 0:
            c = min(left, most)
            r, l = _episodes_of_theta(self.engine, c, tslimit, rs)
            rets.append(r); lens.append(l); bcs.append(self.engine.dense_bc(c))
            left -= c
        self.archive_append(np.mean(np.concatenate(bcs).astype(np.float64), axis=0).astype(np.float32).reshape(1, -1))
        return np.concatenate(rets), np.concatenate(lens)


def _is_dense_run(engine, exp):
    """main's routing: a caller's KIND_DENSE engine; without an engine LinearClassifier on the maze, the cart-pole or the acrobot, and
    SimpleClassifier on the acrobot (which has no kind of its own).  Everything else is the
    maze path's, which refuses what it always refused."""
    if engine is not None:
        return engine.kind == _lib.KIND_DENSE
    return (exp.get('model') == LINEAR_MODEL and exp.get('game') in ('maze', CARTPOLE_GAME, ACROBOT_GAME)) or \
        (exp.get('model') == acrobot_run.SIMPLE_MODEL and exp.get('game') == ACROBOT_GAME)


def _check_dense(engine, exp):
    """a caller's KIND_DENSE engine against exp['game'] and exp['model']"""
    game, asked = exp.get('game'), exp.get('model')
    if engine is None:
        return
    if DENSE_GAMES.get(engine.env_kind) != game:
        raise ValueError("game {!r} asked for, the engine passed in (kind {} on environment kind {}) runs {!r}".format(
            game, engine.kind, engine.env_kind, DENSE_GAMES.get(engine.env_kind)))
    if engine.env_kind == _lib.KIND_PENDULUM:
        raise NotImplementedError("game {!r}: this loop runs a KIND_DENSE engine on 'maze' and {!r}".format(game, CARTPOLE_GAME))
    if asked is not None and asked != ((acrobot_run.simple_name(engine, asked) if acrobot_run.is_engine(engine) else None) or dense_model_name(engine)):
        raise ValueError("model {!r} asked for, the engine passed in (kind {}) runs {!r}".format(asked, engine.kind, dense_model_name(engine)))


def main(log_dir, engine=None, noise=None, seed=0, max_iters=None, **exp):
    """Returns the NsesState (thetas, optimizer states and archive pulled from the device)."""
    from . import tabular_logger as tlogger
    tlogger.start(log_dir)
    dense =_is_dense_run(engine, exp)
    if dense:
        _check_dense(engine, exp)
    else:
        if exp.get('game') != 'maze' or exp.get('model') != MAZE_MODEL:
            raise NotImplementedError("game {!r} with model {!r}: this loop runs game 'maze' with model {!r}".format(exp.get('game'), exp.get('model'), MAZE_MODEL))
        check_engine(engine)
    algo_type = exp['algo_type']
    if algo_type not in ALGO_TYPES:
        raise ValueError("algo_type {!r}: expected one of {}".format(algo_type, ALGO_TYPES))
    ns = exp['novelty_search']
    M, k, method = int(ns['population_size']), int(ns['k']), ns['selection_method']
    R = int(ns['num_rollouts'])
    if dense and exp.get('game') in (CARTPOLE_GAME, ACROBOT_GAME):
        if R < 1:
            raise ValueError("num_rollouts {!r}: at least one episode forms a behaviour characterisation".format(ns['num_rollouts']))
    elif R != 1:
        raise ValueError("num_rollouts {!r}: the maze is deterministic, every rollout of a theta ends at the same point; 1 is the one value".format(ns['num_rollouts']))
    if method not in SELECTION_METHODS:
        raise NotImplementedError(method)                           # nses.py:305-306
    if exp['return_proc_mode'] not in PROC_MODES:
        raise NotImplementedError(exp['return_proc_mode'])          # nses.py:223-224
    if M < 1 or not 1 <= k <= _lib.MAZE_NOVELTY_KMAX:
        raise ValueError("novelty_search: population_size {} and k {} (1 <= k <= {})".format(M, k, _lib.MAZE_NOVELTY_KMAX))
    n_pairs = exp['population_size'] // 2
    side = (_DenseSide if dense else _MazeSide)(exp, engine, noise, max(2 * n_pairs, M, 2))
    engine, noise = side.engine, side.noise
    rs = np.random.RandomState(seed)
    all_tstart = time.time()
    _, _, _, tslimit_max, _ = parse_cutoff(exp['episode_cutoff_mode'])
    try:
        with open(os.path.join(log_dir, 'snapshot.pkl'), 'rb') as file:
            state = pickle.load(file)
        was_algo = getattr(state, 'algo', 'es_gpu')
        if was_algo != ALGO:
            raise ValueError("snapshot.pkl in {} was written by {!r}; this run is {!r}".format(log_dir, was_algo, ALGO))
        was, now = (state.algo_type, state.pop_size, state.k), (algo_type, M, k)
        if was != now:
            raise ValueError("snapshot.pkl in {} holds algo_type {!r}, population_size {}, k {}; this run is algo_type {!r}, population_size {}, k {}".format(
                log_dir, *(was + now)))
        was = (getattr(state, 'game', 'maze'), getattr(state, 'model', MAZE_MODEL), state.num_params, getattr(state, 'num_rollouts', 1))
        now = (side.game, side.model, engine.P, R)
        if was != now:
            raise ValueError("snapshot.pkl in {} holds game {!r}, model {!r}, P = {}, num_rollouts {}; this run is game {!r}, model {!r}, P = {}, num_rollouts {}".format(
                log_dir, *(was + now)))
        tlogger.log("Loaded iteration {} from {}".format(state.it, log_dir))
        side.archive_clear()
        side.archive_append(state.archive)
        rs.set_state(state.stream)
    except FileNotFoundError:
        state = NsesState(exp, M, k)
        state.game, state.model, state.num_params = side.game, side.model, engine.P
        if dense:
            state.num_rollouts = R                                   # (the maze path's snapshot keeps its attributes: it runs 1 and nothing else)
        side.archive_clear()
        for m in range(M):                                           # nses.py:95-117
            idx = noise.sample_index(rs, engine.P)
            theta = noise.get(idx, engine.P) * side.scale_by
            engine.set_theta(theta)
            side.episodes_to_archive(R, tslimit_max, rs)
            state.thetas.append(np.array(theta, np.float32))
            state.optimizers.append((np.zeros(engine.P, np.float32), np.zeros(engine.P, np.float32), 0))
        state.archive = side.archive()
        state.stream = rs.get_state()
    iters = 0
    while max_iters is None or iters < max_iters:
        iters += 1
        tstart_iteration = time.time()
        if state.timesteps_so_far >= exp['timesteps']:
            break
        p = state.curr_parent
        _push_parent(engine, state.thetas[p], state.optimizers[p])
        power = state.mutation_power.value(iteration=state.it, timesteps_so_far=state.timesteps_so_far)
        idx = np.array([noise.sample_index(rs, engine.P) for _ in range(n_pairs)], np.int64)
        seeds = rs.randint(0, 2 ** 32, size=2 * n_pairs, dtype=np.uint64).astype(np.uint32)
        limit = side.step_limit(state.tslimit)
        rets, _, lens = engine.es_eval(idx, power, limit, seeds)
        novelty = sanitized(side.novelty(k, n=2 * n_pairs))
        aux = novelty.astype(np.float32)
        aux[~np.isfinite(aux)] = 0.0                                 # (a finite double beyond float32's range)
        rec = pack_records(idx, rets, lens, aux.reshape(-1, 2))
        update_ratio = nses.blend_and_update(engine, rec, algo_type, exp['return_proc_mode'], exp['l2coeff'], exp['optimizer'])
        test_ret, test_len = side.episodes_to_archive(R, tslimit_max, rs)       # nses.py:246-247
        state.thetas[p] = engine.get_theta()                        # nses.py:288-289
        state.optimizers[p] = engine.optimizer_get_state()
        state.parents.append(p)
        state.novelty_log.append((float(novelty.mean()), float(novelty.max())))
        state.it += 1
        timesteps_this_iter = int(np.sum(lens))
        state.timesteps_so_far += timesteps_this_iter
        state.num_frames += timesteps_this_iter
        if state.adaptive_tslimit and (np.asarray(lens) == state.tslimit).mean() >= state.incr_tslimit_threshold:   # nses.py:250-253
            state.tslimit = min(int(state.tslimit_incr_ratio * state.tslimit), int(state.tslimit_max))
        state.curr_parent = select_parent(engine, state, method, k, limit, rs, side.novelty)
        state.archive = side.archive()
        time_elapsed_this_iter = time.time() - tstart_iteration
        state.time_elapsed += time_elapsed_this_iter
        for key, val in (('Iteration', state.it), ('ParentId', p), ('MutationPower', power), ('TimestepLimitPerEpisode', state.tslimit),
                         ('EpRewMean', np.mean(rets)), ('EpRewMax', np.max(rets)), ('EpLenMean', np.mean(lens)),
                         ('NoveltyMean', state.novelty_log[-1][0]), ('NoveltyMax', state.novelty_log[-1][1]),
                         ('ArchiveSize', int(state.archive.shape[0])), ('UpdateRatio', float(update_ratio)),
                         ('TestRew', float(test_ret[0])), ('TestEpLen', int(test_len[0])),
                         ('TimestepsThisIter', timesteps_this_iter), ('TimestepsPerSecondThisIter', timesteps_this_iter / max(time_elapsed_this_iter, 1e-9)),
                         ('TimestepsSoFar', state.timesteps_so_far), ('TimeElapsedThisIter', time_elapsed_this_iter),
                         ('TimeElapsed', state.time_elapsed), ('TimeElapsedTotal', time.time() - all_tstart)):
            tlogger.record_tabular(key, val)
        tlogger.dump_tabular()
        state.stream = rs.get_state()
        os.makedirs(log_dir, exist_ok=True)
        with open(os.path.join(log_dir, 'snapshot.pkl'), 'wb') as file:
            pickle.dump(state, file)
        if state.timesteps_so_far >= exp['timesteps']:
            break
    return state
