"""The Deep-GA loop of the reference's GPU tree (gpu_implementation/ga.py) on the HIP engine: mutation-power schedules
(neuroevolution/helper.py:46-88), TrainingState / Offspring with `snapshot.pkl` resume (ga.py:40-112, 135-143, 251-256),
genomes ((idx0,), (idx1, power1), ...) with a scaled-noise root (models/base.py:118-149), truncation selection with a
validated elite (ga.py:166-204, 263-274).

Models: `Model` (models/dqn.py:24-37: conv 16 8x8/4, conv 32 4x4/2, fc 256, out) -- its forward is the engine's GAAtariPolicy
network -- and `LargeModel` (dqn.py:39-47: conv 32/64/64, fc 512, the one configurations/ga_atari_config.json names), the engine's
DNE_KIND_GA_LARGE (csrc/forward_large.h); exp['model'] picks one like ga.py:110.
The reference evaluates through TensorFlow workers (ConcurrentWorkers.monitor_eval); here a generation is one
dne_ga_eval_powers call and the validation / test episodes are batched calls of the same entry point.
Unseeded streams of the reference (np.random.RandomState() in ga.py:127, the environments' own seeds) are seeded here.

exp['game'] == 'maze' with exp['model'] == 'SimpleClassifier' (gym_tensorflow.make's first branch, models/simple.py:29-35) runs maze_main below on
a DNE_KIND_MAZE engine: the parents live in a bank on the device, a member is a (parent, noise index, power) triple that k_maze_rollout
evaluates as it stands, selected children become parents device to device (dne_maze_ga_promote), and genomes are written out only for the
few individuals that survive a generation.  SimpleClassifier on an Atari game and the Atari models on the maze are refused.
With exp['novelty_search'] = {'k': ..., 'archive_prob': ...} the maze loop is GA-NS (maze_ns_main): the same GA selecting on novelty against the
archive and the current population, scored on the device (k_maze_novelty_pool).  The key on an Atari game is refused.
A dense policy of any small shape on the maze or the cart-pole runs dense_main on a DNE_KIND_DENSE engine (csrc/dense_ga.h, DESIGN.md section
17a): exp['model'] == 'LinearClassifier' on 'maze' or 'gym.CartPole-v1', 'SimpleClassifier' on 'gym.CartPole-v1' (hidden (16, 16): the GPU tree's
gym configuration), or a caller's engine of kind KIND_DENSE of any shape on its environment's game.  It is maze_main's loop -- _bank_loop, one text
for both -- on dense_ga_build / dense_ga_eval / dense_ga_promote; selection_threshold 0 is random search.  Every other kind of engine with these
models or games is refused as before.
GA-NS on a dense policy is dense_ns_main, called directly (main and dense_main refuse exp['novelty_search'] on a dense run): maze_ns_main's loop on the
dense bank, novelty over final states scored on the device (k_dense_novelty_pool).
GA-NS on an Atari game is atari_ns_main, called directly as well (main keeps refusing exp['novelty_search'] there): main's Atari evaluation under
the same loop, novelty over final RAM states scored on the device (k_ram_novelty_pool).
There are three generation loops: main's Atari loop, _bank_loop (maze_main and dense_main, over a _MazeBank or a _DenseBank) and _ns_loop (maze_ns_main,
dense_ns_main and atari_ns_main, over a _BankNs around one of the two banks or an _AtariNs; its docstring holds GA-NS's decisions).  They share what is
the same in them as plain functions: all three _validate_and_test, _record_rows and _end_generation; _bank_loop and _ns_loop also _resume and
_draw_generation, and _member, _promote and _bank_evaluate where there is a bank; the GA-NS drivers _check_ns; dense_main and dense_ns_main the
engine's opening, _open_dense_run, maze_main and maze_ns_main _open_maze_run.  The maze's engine, walls and noise table come from maze_run.open_engine.
"""
import math
import numbers
import os
import pickle
import time

import numpy as np

from . import _lib, policies, tabular_logger as tlogger
from .es import SharedNoiseTable, parse_cutoff
from .maze_run import MAZE_MODEL, open_engine, step_limit
from .policies import flat_layout


# ---------------------------------------------------------------------------------------------- mutation-power schedules
class Schedule(object):
    """The three schedules of neuroevolution/helper.py:46-88 as one value object.  The experiment JSON names them by the
    reference's class names ('ConstantSchedule', 'LinearSchedule', 'ExponentialSchedule') with that class's keyword arguments;
    progress is looked up by `field` among the keywords of value() ('iteration', 'timesteps_so_far': ga.py:73-74).
    linear:       start + min(progress / span, 1) * (stop - start)
    exponential:  the same interpolation between log(start) and log(stop), exponentiated.  (The reference's
                  ExponentialSchedule.value calls `self.linear(**kwargs)` on an object without __call__ and raises; the
                  interpolation in log space is what its constructor sets up.)"""
    KINDS = {'ConstantSchedule': 'constant', 'LinearSchedule': 'linear', 'ExponentialSchedule': 'exponential'}

    def __init__(self, kind, start, stop=None, span=None, field=None):
        if kind not in ('constant', 'linear', 'exponential'):
            raise ValueError('unknown schedule kind {!r}'.format(kind))
        self.kind, self.start, self.stop, self.span, self.field = kind, start, stop, span, field

    @classmethod
    def from_config(cls, spec):
        """helper.py:84-88: a bare number is a constant; otherwise {'type': <reference class name>, ...its keyword arguments}"""
        if isinstance(spec, numbers.Number):
            return cls('constant', spec)
        kw = dict(spec)
        kind = cls.KINDS[kw.pop('type')]
        if kind == 'constant':
            return cls(kind, kw['value'])
        return cls(kind, kw['initial_p'], kw['final_p'], kw['schedule'], kw['field'])

    def value(self, **progress):
        if self.kind == 'constant':
            return self.start
        # the reference asserts here (helper.py:61); callers that catch its AssertionError keep working
        assert self.field in progress, 'schedule needs {!r}; value() was given {}'.format(self.field, sorted(progress))
        reached = min(float(progress[self.field]) / self.span, 1.0)
        if self.kind == 'linear':
            return self.start + reached * (self.stop - self.start)
        lo, hi = math.log(self.start), math.log(self.stop)
        return math.exp(lo + reached * (hi - lo))


make_schedule = Schedule.from_config


class _LegacySchedule(Schedule):
    """snapshot.pkl files written before the three schedule classes became one hold TrainingState.mutation_power as an instance of
    dne_hip.ga_gpu.ConstantSchedule / LinearSchedule / ExponentialSchedule with those classes' own attributes (helper.py:46-82's:
    _value -- or schedule, field, initial_p, final_p).  These names keep such files loadable: unpickling hands the old attribute
    dict to __setstate__, which maps it onto Schedule's."""
    KIND = None

    def __init__(self, *args, **kw):
        spec = dict(kw, type=type(self).__name__)
        if args:                                   # the old positional forms: (value) / keyword-only otherwise
            spec['value'] = args[0]
        fresh = Schedule.from_config(spec)
        self.__dict__.update(fresh.__dict__)

    def __setstate__(self, state):
        if 'kind' in state:                        # written after the merge
            self.__dict__.update(state)
        elif self.KIND == 'constant':
            Schedule.__init__(self, 'constant', state['_value'])
        else:                                      # the old ExponentialSchedule also carried a helper object (`linear`): not needed
            Schedule.__init__(self, self.KIND, state['initial_p'], state['final_p'], state['schedule'], state['field'])


class ConstantSchedule(_LegacySchedule):
    KIND = 'constant'


class LinearSchedule(_LegacySchedule):
    KIND = 'linear'


class ExponentialSchedule(_LegacySchedule):
    KIND = 'exponential'


# ---------------------------------------------------------------------------------------------- run state (what snapshot.pkl holds)
class Offspring(object):
    """One evaluated genome (ga.py:88-106): seeds = (idx0, (idx1, power1), ...), the rewards / lengths of its training
    episodes and -- once validated -- of its validation episodes."""

    def __init__(self, seeds, rewards, ep_len, validation_rewards=(), validation_ep_len=()):
        self.seeds = seeds
        self.rewards, self.ep_len = rewards, ep_len
        self.validation_rewards, self.validation_ep_len = list(validation_rewards), list(validation_ep_len)

    fitness = property(lambda self: np.mean(self.rewards))
    training_steps = property(lambda self: np.sum(self.ep_len))


class TrainingState(object):
    """Everything a run needs to continue after a restart (ga.py:40-76): counters, the sorted population, the elite, the best
    validated solution, the mutation-power schedule and the episode cutoff with its adaptive growth rule."""
    COUNTERS = ('num_frames', 'timesteps_so_far', 'time_elapsed', 'validation_timesteps_so_far', 'it')

    def __init__(self, exp):
        for name in self.COUNTERS:
            setattr(self, name, 0)
        self.population, self.elite = [], None
        self.curr_solution, self.curr_solution_val, self.curr_solution_test = None, float('-inf'), float('-inf')
        self.mutation_power = Schedule.from_config(exp['mutation_power'])
        limit, grow_at, grow_by, limit_max, adaptive = parse_cutoff(exp['episode_cutoff_mode'])
        self.tslimit, self.adaptive_tslimit = limit, adaptive
        self.incr_tslimit_threshold, self.tslimit_incr_ratio = grow_at, grow_by
        if adaptive:
            self.tslimit_max = limit_max

    def sample(self, schedule):
        return schedule.value(iteration=self.it, timesteps_so_far=self.timesteps_so_far)

    def copy_population(self, filename):
        """Start from another run's population (exp['load_population'], ga.py:78-86).  Snapshots written before mutation powers
        were stored per seed hold bare indices: those mutations were made at power 0.005."""
        with open(filename, 'rb') as f:
            self.population = pickle.load(f).population
        for o in self.population:
            root, rest = o.seeds[0], o.seeds[1:]
            o.seeds = (root, ) + tuple(m if isinstance(m, tuple) else (m, 0.005) for m in rest)


# ---------------------------------------------------------------------------------------------- models/dqn.py:24-37, base.py:190-201
def model_scale_by(nact, kind=None):
    """scale_by of `Model` / `LargeModel` (dqn.py:25-27, inherited by LargeModel): weights std / sqrt(prod(shape[:-1])) with std 1.0
    (out layer 0.1), biases 0 -- in the engine's flat order = the creation order of dqn.py:29-36 / 39-47."""
    spec, P = flat_layout(_lib.KIND_GA if kind is None else kind, nact)
    sb = np.zeros(P, np.float32)
    for name, (off, shape) in spec.items():
        n = int(np.prod(shape))
        if name.endswith('/w'):
            std = 0.1 if name.startswith('out') else 1.0
            sb[off:off + n] = np.float32(std / np.sqrt(np.prod(shape[:-1])))
    return sb


MODEL_KINDS = {'Model': _lib.KIND_GA, 'LargeModel': _lib.KIND_GA_LARGE}   # neuroevolution/models/dqn.py:24-47 (exp['model'], ga.py:110)
ALGO = 'ga'                              # what maze_main's snapshot.pkl says wrote it
ALGO_NS = 'ga_ns'                        # ... and maze_ns_main's
NS_KEY = 'novelty_search'                # exp[NS_KEY] = {'k': neighbours, 'archive_prob': chance of a member to enter the archive}


class HipModel(object):
    """randomize / mutate / compute_weights_from_seeds of models/base.py:113-149, with theta living on the device"""

    def __init__(self, engine):
        self.engine, self.num_params = engine, engine.P
        self.scale_by = model_scale_by(engine.n_actions, engine.kind)
        engine.ga_set_init_scale(self.scale_by)

    def randomize(self, rs, noise):
        return (noise.sample_index(rs, self.num_params), )

    def mutate(self, parent_seeds, rs, noise, mutation_power):
        return tuple(parent_seeds) + ((noise.sample_index(rs, self.num_params), mutation_power), )

    def compute_weights_from_seeds(self, noise, seeds, cache=None):
        return self.engine.ga_rebuild_powers(0, seeds)


def _evaluate(engine, genomes, tslimit, rs):
    """(returns, lengths) of one episode per genome; env seeds from `rs` (the reference's environments are unseeded)"""
    limit = _lib.ENV_MAX_EPISODE_STEPS if tslimit is None else min(int(tslimit), _lib.ENV_MAX_EPISODE_STEPS)
    out_r, out_l = [], []
    for s in range(0, len(genomes), engine.max_members):
        part = genomes[s:s + engine.max_members]
        ret, _, ln = engine.ga_eval_powers(part, limit, rs.randint(0, 2 ** 32, size=len(part), dtype=np.uint64).astype(np.uint32))
        out_r.append(ret); out_l.append(ln)
    return np.concatenate(out_r), np.concatenate(out_l)


def parents_of(state, T):
    """ga.py:147-156, 263-274: the genomes of the next parents -- the top T, the elite first in place of the last if it is not among them"""
    if not state.population or T <= 0:
        return []
    top = [o.seeds for o in state.population[:T]]
    if state.elite is None or state.elite.seeds in top:
        return top
    return [state.elite.seeds] + top[:T - 1]


# ---------------------------------------------------------------------------------------------- what the three loops below share
def _validate_and_test(state, exp, validation_population, evaluate, population_timesteps):
    """ga.py:184-201, 223-226 behind a generation's evaluation: the validation episodes of validation_population, the best of them as the
    new state.elite, its test episodes (max_frames=None), the timestep counters and curr_solution_*.  evaluate(individuals, tslimit) ->
    (returns, lengths), one episode per Offspring of the list.  Returns what the tabular rows need."""
    k = exp['num_validation_episodes']
    vr, vl = evaluate([o for o in validation_population for _ in range(k)], state.tslimit)        # ga.py:188-192
    population_validation = [float(np.mean(vr[i * k:(i + 1) * k])) for i in range(len(validation_population))]
    validation_timesteps = sum(int(np.sum(vl[i * k:(i + 1) * k])) for i in range(len(validation_population)))
    state.elite = validation_population[int(np.argmax(population_validation))]                    # ga.py:198-199
    er, el = evaluate([state.elite] * exp['num_test_episodes'], None)                             # ga.py:200-201
    timesteps_this_iter = population_timesteps + validation_timesteps
    state.timesteps_so_far += timesteps_this_iter
    state.validation_timesteps_so_far += validation_timesteps
    if np.mean(population_validation) > state.curr_solution_val:                                  # ga.py:223-226
        state.curr_solution = state.elite.seeds
        state.curr_solution_val = float(np.mean(population_validation))
        state.curr_solution_test = float(np.mean(er))
    return dict(validation_population=validation_population, population_validation=population_validation, validation_timesteps=validation_timesteps,
                timesteps_this_iter=timesteps_this_iter, population_timesteps=population_timesteps, er=er, el=el)


def _record_rows(state, power, rewards, T, v, dt, all_tstart):
    """the tabular rows of a GA generation (ga.py:206-241), recorded and not yet dumped; v is what _validate_and_test returned"""
    for key, val in (('Iteration', state.it), ('MutationPower', power), ('PopulationEpRewMax', np.max(rewards)),
                     ('PopulationEpRewMean', np.mean(rewards)), ('PopulationEpCount', len(rewards)),
                     ('PopulationTimesteps', v['population_timesteps']), ('NumSelectedIndividuals', T),
                     ('TruncatedPopulationRewMean', np.mean([a.fitness for a in v['validation_population']])),
                     ('TruncatedPopulationValidationRewMean', np.mean(v['population_validation'])),
                     ('TruncatedPopulationEliteValidationRewMean', np.max(v['population_validation'])),
                     ('TruncatedPopulationEliteTestRewMean', np.mean(v['er'])), ('TruncatedPopulationEliteTestEpCount', len(v['er'])),
                     ('TruncatedPopulationEliteTestEpLenSum', int(np.sum(v['el']))), ('ValidationTimestepsThisIter', v['validation_timesteps']),
                     ('TimestepsThisIter', v['timesteps_this_iter']), ('TimestepsPerSecondThisIter', v['timesteps_this_iter'] / dt),
                     ('TimestepsSoFar', state.timesteps_so_far), ('TimeElapsedThisIter', dt), ('TimeElapsed', state.time_elapsed),
                     ('TimeElapsedTotal', time.time() - all_tstart)):
        tlogger.record_tabular(key, val)


def _end_generation(state, log_dir, lens, rs=None):
    """ga.py:244-254: the adaptive cutoff's step on this generation's episode lengths, then snapshot.pkl -- with the position of rs, where
    the loop's stream is seeded and a resume continues it"""
    if state.adaptive_tslimit:
        if np.mean(np.asarray(lens) >= state.tslimit) > state.incr_tslimit_threshold:
            state.tslimit = min(state.tslimit * state.tslimit_incr_ratio, state.tslimit_max)
    if rs is not None:
        state.stream = rs.get_state()
    os.makedirs(log_dir, exist_ok=True)
    with open(os.path.join(log_dir, 'snapshot.pkl'), 'wb') as file:
        pickle.dump(state, file)


def main(log_dir, engine=None, noise=None, seed=0, max_iters=None, **exp):
    """gpu_implementation/ga.py:114-275.  Returns (curr_solution_test, {'val': curr_solution_val}, state).

    exp['novelty_search'] runs GA-NS on game 'maze' under 'SimpleClassifier' (maze_ns_main).  On a dense run it raises NotImplementedError:
    GA-NS on a dense policy is dense_ns_main, called directly."""
    maze, asked = exp.get('game') == 'maze', exp.get('model', 'Model')
    if _is_dense_run(engine, exp):                                  # a dense policy on a step environment: the bank of csrc/dense_ga.h
        return dense_main(log_dir, engine=engine, noise=noise, seed=seed, max_iters=max_iters, **exp)
    if maze != (asked == MAZE_MODEL):                               # ga.py:110-114 takes any pair; the engine has these
        raise NotImplementedError("model {!r} on game {!r}: {!r} runs on game 'maze' only, and 'maze' runs nothing else".format(
            asked, exp.get('game'), MAZE_MODEL))
    if maze:
        return maze_main(log_dir, engine=engine, noise=noise, seed=seed, max_iters=max_iters, **exp)
    if NS_KEY in exp:
        raise NotImplementedError("game {!r} with exp[{!r}]: GA-NS runs on game 'maze' only".format(exp.get('game'), NS_KEY))
    tlogger.start(log_dir)
    if engine is None:
        engine = _lib.Engine(MODEL_KINDS[exp.get('model', 'Model')], 18, max_members=exp['population_size'])
    noise = noise if noise is not None else SharedNoiseTable()
    noise.attach(engine)
    model = HipModel(engine)
    rs = np.random.RandomState(seed)
    all_tstart = time.time()
    try:                                                           # ga.py:135-143: resume
        with open(os.path.join(log_dir, 'snapshot.pkl'), 'rb+') as file:
            state = pickle.load(file)
        tlogger.log("Loaded iteration {} from {}".format(state.it, log_dir))
        if getattr(state, 'game', None) == 'maze':
            raise ValueError("snapshot.pkl in {} holds game 'maze' under model {!r}; this run is game {!r} under model {!r}".format(
                log_dir, getattr(state, 'model', None), exp.get('game'), asked))
    except FileNotFoundError:
        state = TrainingState(exp)
    if 'load_population' in exp:
        state.copy_population(exp['load_population'])

    def evaluate(individuals, tslimit):
        return _evaluate(engine, [o.seeds for o in individuals], tslimit, rs)

    cached_parents = parents_of(state, exp['selection_threshold'])
    iters = 0
    while max_iters is None or iters < max_iters:
        iters += 1
        tstart_iteration = time.time()
        if state.timesteps_so_far >= exp['timesteps']:
            break
        assert (len(cached_parents) == 0 and state.it == 0) or len(cached_parents) == exp['selection_threshold']
        power = state.sample(state.mutation_power)
        tasks = [model.randomize(rs, noise) if not cached_parents else
                 model.mutate(cached_parents[rs.randint(len(cached_parents))], rs, noise, mutation_power=power)
                 for _ in range(exp['population_size'])]                                       # ga.py:128-133, 161
        rets, lens = _evaluate(engine, tasks, state.tslimit, rs)
        results = [Offspring(s, [float(r)], [int(l)]) for s, r, l in zip(tasks, rets, lens)]    # ga.py:162-163
        state.num_frames += int(lens.sum()) * 4
        state.it += 1
        rewards = np.array([a.fitness for a in results])
        # ga.py:176: sorted(..., reverse=True) is stable, so equal fitness keeps arrival order -- the engine's selection
        # order (-fitness, arrival index)
        order = engine.ga_select(rewards.astype(np.float32), len(results))
        state.population = [results[i] for i in order]
        validation_population = state.population[:exp['validation_threshold']]                # ga.py:184-186
        if state.elite is not None:
            validation_population = [state.elite] + validation_population[:-1]
        v = _validate_and_test(state, exp, validation_population, evaluate, sum(a.training_steps for a in results))
        dt = time.time() - tstart_iteration
        state.time_elapsed += dt
        _record_rows(state, power, rewards, exp['selection_threshold'], v, dt, all_tstart)
        tlogger.dump_tabular()
        _end_generation(state, log_dir, lens)
        if state.timesteps_so_far >= exp['timesteps']:
            break
        cached_parents = parents_of(state, exp['selection_threshold'])                          # ga.py:261-274
    return float(state.curr_solution_test), {'val': float(state.curr_solution_val)}, state


# ---------------------------------------------------------------------------------------------- the hard maze
KEPT = -1          # a descriptor's noise index that means "the parent itself" (dne_maze_ga_promote)


class _MazeBank(object):
    """the device bank of a KIND_MAZE engine as the loops below call it: build(genomes), promote(parent, idx, power) and
    eval(parent, idx, power, tslimit) -> (returns, lengths), tslimit None meaning the environment's own limit.  For GA-NS, archive() names
    the engine's archive calls as _BankNs takes them: clear, append, novelty_pool, append_members, the whole read-back, and the empty archive"""

    def __init__(self, engine):
        self.engine, self.max_members = engine, engine.max_members
        self.build, self.promote = engine.maze_ga_build, engine.maze_ga_promote

    def eval(self, parent, idx, power, tslimit):
        ret, _, ln = self.engine.maze_ga_eval(parent, idx, power, step_limit(tslimit))
        return ret, ln

    def archive(self):
        e = self.engine
        return (e.maze_archive_clear, e.maze_archive_append, e.maze_novelty_pool, e.maze_archive_append_members, e.maze_archive,
                np.zeros((0, 2), np.float32))


class _DenseBank(object):
    """the same three calls on a KIND_DENSE engine (dense_ga_*).  On the cart-pole and the acrobot every eval draws its members' environment seeds from rs,
    after whatever its caller drew; on the maze nothing is drawn"""

    def __init__(self, engine, rs):
        self.engine, self.max_members, self.rs = engine, engine.max_members, rs
        self.build, self.promote = engine.dense_ga_build, engine.dense_ga_promote
        self.own = {_lib.KIND_MAZE: _lib.MAZE_STEPS, _lib.ENV_ACROBOT: _lib.ACROBOT_STEPS}.get(engine.env_kind, _lib.CARTPOLE_STEPS)

    def eval(self, parent, idx, power, tslimit):
        seeds = None
        if self.engine.env_kind != _lib.KIND_MAZE:
            seeds = self.rs.randint(0, 2 ** 32, size=len(parent), dtype=np.uint64).astype(np.uint32)
        ret, _, ln = self.engine.dense_ga_eval(parent, idx, power, self.own if tslimit is None else min(int(tslimit), self.own), seeds)
        return ret, ln

    def archive(self):
        e = self.engine
        return (e.dense_archive_clear, e.dense_archive_append, e.dense_novelty_pool, e.dense_archive_append_members, e.dense_archive,
                np.zeros((0, e.dense_bc_dim()), np.float32))


def _bank_evaluate(bank, members, tslimit):
    """(returns, lengths) of one episode per (parent, idx, power) member, in calls of at most max_members"""
    out_r, out_l = [], []
    for s in range(0, len(members), bank.max_members):
        parent, idx, power = zip(*members[s:s + bank.max_members])
        ret, ln = bank.eval(np.array(parent, np.int32), np.array(idx, np.int64), np.array(power, np.float32), tslimit)
        out_r.append(ret); out_l.append(ln)
    return np.concatenate(out_r), np.concatenate(out_l)


def _open_maze_run(log_dir, engine, noise, seed, exp):
    """what maze_main and maze_ns_main do before they look for a snapshot: the log, the engine with walls, table and init scale, the stream"""
    tlogger.start(log_dir)
    engine, noise = open_engine(exp, engine, noise, exp['population_size'])
    engine.maze_ga_set_init_scale(policies.simple_scale_by())
    return engine, noise, np.random.RandomState(seed)


def _resume(log_dir, algo, rs, game='maze', model=MAZE_MODEL, P=None):
    """ga.py:135-143 for a run of `algo` in _bank_loop or _ns_loop (the maze drivers; the others with their game, model and P): the state in log_dir's snapshot.pkl
    with the position of its stream restored into rs, or None if there is no such file.  A snapshot of another driver, game, model or P is
    refused, naming both."""
    try:
        with open(os.path.join(log_dir, 'snapshot.pkl'), 'rb') as file:
            state = pickle.load(file)
    except FileNotFoundError:
        return None
    tlogger.log("Loaded iteration {} from {}".format(state.it, log_dir))
    was_algo = getattr(state, 'algo', ALGO if isinstance(state, TrainingState) else 'es_gpu')
    if was_algo != algo:
        raise ValueError("snapshot.pkl in {} was written by {!r}; this run is {!r}".format(log_dir, was_algo, algo))
    was = (getattr(state, 'game', None) or 'an Atari game', getattr(state, 'model', 'Model'))
    if was != (game, model):
        raise ValueError("snapshot.pkl in {} holds game {!r} under model {!r}; this run is game {!r} under model {!r}".format(
            log_dir, was[0], was[1], game, model))
    if P is not None and getattr(state, 'num_params', None) != P:
        raise ValueError("snapshot.pkl in {} holds model {!r} with P = {}; this run is model {!r} with P = {}".format(
            log_dir, was[1], getattr(state, 'num_params', None), model, P))
    if getattr(state, 'stream', None) is not None:
        rs.set_state(state.stream)
    return state


def _draw_generation(rs, n, n_parents, indices):
    """a generation's two whole-array draws: the parent of every member (-1: a root, while there are no parents), then its noise index"""
    of = rs.randint(n_parents, size=n).astype(np.int32) if n_parents else np.full(n, -1, np.int32)
    return of, rs.randint(0, indices, size=n).astype(np.int64)


def _member(i, of, idx, power, parents):
    """the descriptor of a generation's member i over the bank as it is, and its genome"""
    i = int(i)
    if of[i] < 0:
        return (-1, int(idx[i]), 0.0), (int(idx[i]), )
    return (int(of[i]), int(idx[i]), float(power)), tuple(parents[of[i]]) + ((int(idx[i]), power), )


def _promote(promote, descriptors):
    """the next bank from descriptors over this one, device to device; promote is the engine's call (maze_ga_promote, dense_ga_promote)"""
    promote(*(np.array(c, t) for c, t in zip(zip(*descriptors), (np.int32, np.int64, np.float32))))


def _bank_loop(log_dir, exp, state, bank, engine, rs, indices, max_iters, all_tstart):
    """maze_main's and dense_main's generations over a device bank (their docstrings say what one is): state is the run's TrainingState, bank
    a _MazeBank or _DenseBank, indices the number of admissible noise indices.  Returns what main returns."""
    n, T, V = exp['population_size'], exp['selection_threshold'], exp['validation_threshold']
    parents = parents_of(state, T)                                  # the genomes of the bank's parents, kept beside it
    if parents:
        bank.build(parents)
    descriptor = {}                                                 # id(Offspring) -> its descriptor over the bank as it is now

    def evaluate(individuals, tslimit):
        return _bank_evaluate(bank, [descriptor[id(o)] for o in individuals], tslimit)

    iters = 0
    while max_iters is None or iters < max_iters:
        iters += 1
        tstart_iteration = time.time()
        if state.timesteps_so_far >= exp['timesteps']:
            break
        assert (len(parents) == 0 and state.it == 0) or len(parents) == T
        power = state.sample(state.mutation_power)
        of, idx = _draw_generation(rs, n, len(parents), indices)
        rets, lens = bank.eval(of, idx, np.full(n, power, np.float32), state.tslimit)
        state.num_frames += int(lens.sum())
        state.it += 1
        rewards = np.asarray(rets, np.float64)
        order = engine.ga_select(np.asarray(rets, np.float32), n)   # (-fitness, arrival index): a stable sort, ties at -500 keep arrival order
        descriptor.clear()
        state.population = []
        for i in order[:max(T, V)]:
            d, genome = _member(i, of, idx, power, parents)
            o = Offspring(genome, [float(rets[i])], [int(lens[i])])
            descriptor[id(o)] = d
            state.population.append(o)
        validation_population = state.population[:V]                # ga.py:184-186
        if state.elite is not None:
            if state.elite.seeds in parents:
                descriptor[id(state.elite)] = (parents.index(state.elite.seeds), 0, 0.0)
            elif len(state.elite.seeds) == 1:                       # selection_threshold 0: no bank, every individual is a root
                root = state.elite.seeds[0]
                descriptor[id(state.elite)] = (-1, int(root[0] if isinstance(root, (tuple, list)) else root), 0.0)
            else:
                raise NotImplementedError("the elite {!r} is not among the {} parents of the bank".format(state.elite.seeds, len(parents)))
            validation_population = [state.elite] + validation_population[:-1]
        old_elite = state.elite
        v = _validate_and_test(state, exp, validation_population, evaluate, int(lens.sum()))
        dt = time.time() - tstart_iteration
        state.time_elapsed += dt
        _record_rows(state, power, rewards, T, v, dt, all_tstart)
        tlogger.dump_tabular()
        # ga.py:261-274 on the device: the next parents from this generation's descriptors, the retained elite as it stands
        new_parents = parents_of(state, T)
        if new_parents and not parents:                             # the start: generation 0's roots become the first bank
            bank.build(new_parents)
        elif new_parents:
            by_genome = {o.seeds: descriptor[id(o)] for o in state.population}
            if old_elite is not None and state.elite is old_elite and state.elite.seeds in parents:
                by_genome[state.elite.seeds] = (parents.index(state.elite.seeds), KEPT, 0.0)
            _promote(bank.promote, [by_genome[g] for g in new_parents])
        parents = new_parents
        _end_generation(state, log_dir, lens, rs)
        if state.timesteps_so_far >= exp['timesteps']:
            break
    return float(state.curr_solution_test), {'val': float(state.curr_solution_val)}, state


def maze_main(log_dir, engine=None, noise=None, seed=0, max_iters=None, **exp):
    """gpu_implementation/ga.py:114-275 with game 'maze' and model 'SimpleClassifier'.  Returns (curr_solution_test, {'val': ...}, state).

    A generation's member i is the triple (parent p_i, noise index idx_i, power) over the device's bank of T parents -- a root (-1, idx_i)
    while there are none -- so a generation is ONE maze_ga_eval of three small arrays.  Its genome, parents[p_i] + ((idx_i, power),), is only
    written out for the top max(selection_threshold, validation_threshold) and the elite: state.population holds just those (the reference
    reads no more of it, ga.py:150-154, 188).  The next parents are made on the device from this generation's descriptors by one
    maze_ga_promote (a retained elite as the kept form); maze_ga_build from whole genomes runs once per call of main: for the first
    bank after generation 0, or before the loop when load_population or a snapshot brought a population.
    Decisions of ours: the reference's stream is unseeded (ga.py:117) and drawn from one offspring at a time; here a generation takes
    rs.randint(T, size=n) for the parents (if there are any), then rs.randint(0, len(noise) - P + 1, size=n) for the indices, as two
    whole-array draws from RandomState(seed), and no environment seeds (the episode is deterministic).  The stream's position is kept in
    snapshot.pkl with game, model and algo = 'ga', so a resumed run continues bit for bit; a resume under another game or model, or from
    a snapshot of es_gpu.main / nses_gpu.main, raises and names both.  A previous elite is evaluated again as (its bank index, idx 0,
    power 0): the child formula, bank + fl(0 * noise).  The elite's test episodes are num_test_episodes identical deterministic episodes
    at the 400-step default, as the reference runs them.  num_frames counts steps (the maze has no frame skip).
    maze_ns_main below (_ns_loop) is the same scaffold (the _helpers above) around another selection."""
    if NS_KEY in exp:
        return maze_ns_main(log_dir, engine=engine, noise=noise, seed=seed, max_iters=max_iters, **exp)
    engine, noise, rs = _open_maze_run(log_dir, engine, noise, seed, exp)
    all_tstart = time.time()
    state = _resume(log_dir, ALGO, rs)
    if state is None:
        state = TrainingState(exp)
    state.game, state.model, state.algo = 'maze', MAZE_MODEL, ALGO
    if 'load_population' in exp:
        state.copy_population(exp['load_population'])
    return _bank_loop(log_dir, exp, state, _MazeBank(engine), engine, rs, len(noise.noise) - engine.P + 1, max_iters, all_tstart)


# ---------------------------------------------------------------------------------------------- a dense policy on a step environment
DENSE_SIMPLE_HIDDEN = (16, 16)           # SimpleClassifier as a dense shape (models/simple.py:29-35): on the cart-pole csrc/cartpole.h's layout, P = 386


def _is_dense_run(engine, exp):
    """main's routing: a caller's KIND_DENSE engine always; without an engine LinearClassifier on the maze or the cart-pole and
    SimpleClassifier on the cart-pole, and both on the acrobot.  An engine of another kind is never a dense run (main refuses it as it always did)."""
    from .es_gpu import ACROBOT_GAME, CARTPOLE_GAME, LINEAR_MODEL
    if engine is not None:
        return engine.kind == _lib.KIND_DENSE
    game, asked = exp.get('game'), exp.get('model')
    return (asked == LINEAR_MODEL and game in ('maze', CARTPOLE_GAME, ACROBOT_GAME)) or (asked == MAZE_MODEL and game in (CARTPOLE_GAME, ACROBOT_GAME))


def _open_dense_run(who, log_dir, engine, noise, exp):
    """what dense_main and dense_ns_main (`who`) do before they look for a snapshot: the routing and its refusals, the log, the engine with
    walls (on the maze), table and init scale.  Returns (engine, noise, game, model)."""
    from . import acrobot_run
    from .es_gpu import ACROBOT_GAME, CARTPOLE_GAME, DENSE_GAMES, LINEAR_MODEL, dense_model_name
    from .maze_run import attach_table, maze_file
    game, asked = exp.get('game'), exp.get('model')
    if engine is None:
        if not _is_dense_run(None, exp):
            raise NotImplementedError("model {!r} on game {!r}: without an engine {} runs {!r} on 'maze' and {!r}, and {!r} on {!r}; both on {!r}".format(
                asked, game, who, LINEAR_MODEL, CARTPOLE_GAME, MAZE_MODEL, CARTPOLE_GAME, ACROBOT_GAME))
        model = asked
        if game == ACROBOT_GAME:
            engine = acrobot_run.make_engine(exp['population_size'], asked)
        else:
            engine = _lib.Engine(_lib.KIND_DENSE, 2, max_members=exp['population_size'], env=_lib.KIND_MAZE if game == 'maze' else _lib.KIND_CARTPOLE,
                                 hidden=DENSE_SIMPLE_HIDDEN if asked == MAZE_MODEL else (), nonlin='relu')
    else:
        if engine.kind != _lib.KIND_DENSE:
            raise ValueError("{} needs an engine of kind KIND_DENSE ({}), the engine passed in is of kind {}".format(who, _lib.KIND_DENSE, engine.kind))
        if DENSE_GAMES.get(engine.env_kind) != game:
            raise ValueError("game {!r} asked for, the engine passed in (kind {} on environment kind {}) runs {!r}".format(
                game, engine.kind, engine.env_kind, DENSE_GAMES.get(engine.env_kind)))
        if engine.env_kind == _lib.KIND_PENDULUM:
            raise NotImplementedError("game {!r}: this loop runs a KIND_DENSE engine on 'maze' and {!r}".format(game, CARTPOLE_GAME))
        model = (acrobot_run.simple_name(engine, asked) if acrobot_run.is_engine(engine) else None) or dense_model_name(engine)
        if asked is not None and asked != model:
            raise ValueError("model {!r} asked for, the engine passed in (kind {}) runs {!r}".format(asked, engine.kind, model))
    tlogger.start(log_dir)
    if engine.env_kind == _lib.KIND_MAZE:
        engine.maze_set_walls(*_lib.load_maze(maze_file(exp)))
    noise = attach_table(engine, noise)
    engine.dense_ga_set_init_scale(policies.dense_scale_by(engine.env_kind, engine.hidden, engine.n_actions))
    return engine, noise, game, model


def dense_main(log_dir, engine=None, noise=None, seed=0, max_iters=None, **exp):
    """gpu_implementation/ga.py:114-275 over a dense policy of any small shape on the maze, the cart-pole or the acrobot (a DNE_KIND_DENSE engine,
    csrc/dense_ga.h): maze_main's loop (_bank_loop) on dense_ga_build / dense_ga_eval / dense_ga_promote.  Returns what main returns.

    The engine: a caller's KIND_DENSE engine of any shape, on its environment's game (es_gpu.DENSE_GAMES; another game, or a model name that
    is not es_gpu.dense_model_name(engine), is a ValueError naming both; the pendulum is not built); without one, exp['model'] ==
    'LinearClassifier' opens an engine with no hidden layer on 'maze' or 'gym.CartPole-v1', and 'SimpleClassifier' on 'gym.CartPole-v1' one of
    hidden (16, 16), relu -- the GPU tree's gym configuration under GA; on 'gym.Acrobot-v1' (acrobot_run; draws, limits and seeds as on the
    cart-pole, own limit 500) both names open their shape, and a (16, 16) relu engine of the caller's is 'SimpleClassifier' when the run asks
    for that name.  The init scale is policies.dense_scale_by of the shape.
    Lazy genomes, one build per call, promotion with the kept form and selection_threshold == 0 (roots every generation, an empty bank:
    random search) are maze_main's, word for word.  Decisions of ours:
      draws        parents and indices are maze_main's two whole-array draws.  On the maze no environment seed is drawn: the stream is
                   maze_main's, so a (16, 16) relu engine on the maze writes the rows maze_main writes.  On the cart-pole EVERY evaluation
                   call -- a generation, each call of the validation episodes, the test episodes -- draws
                   rs.randint(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32) for its n members after the two draws, so each
                   validation and test episode is a different episode.
      limits       a generation and the validation episodes run under state.tslimit, at most the environment's own limit; the elite's
                   test episodes at the environment's own limit (maze 400, cart-pole 500).
      counters     num_frames counts steps (no frame skip).
      snapshot     game, model (es_gpu.dense_model_name(engine), or 'SimpleClassifier' for the (16, 16) cart-pole route), algo = 'ga',
                   num_params = P and the stream's position; a resume continues bit for bit.  A resume under another game, model, P or
                   driver raises and names both.
    exp['novelty_search'] raises NotImplementedError here, as it does from main on a dense run: GA-NS on a dense policy is dense_ns_main below,
    called directly."""
    if NS_KEY in exp:
        raise NotImplementedError("exp[{!r}] with a dense policy: GA-NS runs on game 'maze' under model {!r} only".format(NS_KEY, MAZE_MODEL))
    engine, noise, game, model = _open_dense_run('dense_main', log_dir, engine, noise, exp)
    rs = np.random.RandomState(seed)
    all_tstart = time.time()
    state = _resume(log_dir, ALGO, rs, game, model, engine.P)
    if state is None:
        state = TrainingState(exp)
    state.game, state.model, state.algo, state.num_params = game, model, ALGO, engine.P
    if 'load_population' in exp:
        state.copy_population(exp['load_population'])
    return _bank_loop(log_dir, exp, state, _DenseBank(engine, rs), engine, rs, len(noise.noise) - engine.P + 1, max_iters, all_tstart)


# ---------------------------------------------------------------------------------------------- GA-NS: one loop, one side object per family
def _check_ns(exp, kmax_name):
    """(k, archive_prob) of exp['novelty_search'], k within 1 .. _lib.<kmax_name> (the family's limit: the message names it)"""
    ns = exp[NS_KEY]
    k, prob, kmax = int(ns['k']), float(ns['archive_prob']), getattr(_lib, kmax_name)
    if not 1 <= k <= kmax:
        raise ValueError("novelty_search k = {}: expected 1 .. {} = {}".format(k, kmax_name, kmax))
    if not 0.0 <= prob <= 1.0:
        raise ValueError("novelty_search archive_prob = {!r}: expected a probability".format(ns['archive_prob']))
    return k, prob


class _BankNs(object):
    """what _ns_loop asks of a family, for the two whose parents live in a device bank (a _MazeBank or a _DenseBank, which also names its engine's
    archive calls): a member is a descriptor over the bank, its genome is written out only for an Offspring, and the whole archive is read back"""
    frames, goal_row = 1, True                                      # num_frames counts steps; BestDistanceToGoal is written (on every game)

    def __init__(self, bank):
        self.bank, self.build = bank, bank.build
        self.clear, self.append, self.novelty_pool, self._append_members, self._read, self.empty = bank.archive()
        self.descriptor = {}                                        # id(Offspring) -> its descriptor over the bank as it is now

    def generation(self, of, idx, power, parents, tslimit):
        self.descriptor.clear()
        self.drawn = (of, idx, power, parents)
        return self.bank.eval(of, idx, np.full(len(of), power, np.float32), tslimit)

    def append_members(self, members, archive):
        if members.size:
            self._append_members(members)
        return self._read()

    def offspring(self, i, ret, length):
        d, genome = _member(i, *self.drawn)
        o = Offspring(genome, [ret], [length])
        self.descriptor[id(o)] = d
        return o

    def evaluate(self, individuals, tslimit):
        return _bank_evaluate(self.bank, [self.descriptor[id(o)] for o in individuals], tslimit)

    def next_parents(self, selected, had_parents):
        """the top T by novelty on the device: every one a root (generation 0, built once) or a child of the bank as it is"""
        if selected and not had_parents:
            self.build([o.seeds for o in selected])
        elif selected:
            _promote(self.bank.promote, [self.descriptor[id(o)] for o in selected])


class _AtariNs(object):
    """the same of an Atari engine created with record_bc: a member is its written-out genome (ga_eval_powers takes genomes, the store keeps the
    parents' vectors cached, so there is no bank to build or promote), and only the appended points are read back"""
    frames, goal_row = 4, False                                     # num_frames counts 4 frames a step; no BestDistanceToGoal

    def __init__(self, engine, rs):
        self.engine, self.rs = engine, rs
        self.clear, self.append, self.novelty_pool = engine.archive_clear, engine.archive_append_points, engine.ram_novelty_pool
        self.empty = np.zeros((0, _lib.RAM_BYTES), np.uint8)

    def build(self, parents):
        pass

    def generation(self, of, idx, power, parents, tslimit):
        self.tasks = [_member(i, of, idx, power, parents)[1] for i in range(len(of))]
        return _evaluate(self.engine, self.tasks, tslimit, self.rs)     # one call: n <= max_members

    def append_members(self, members, archive):
        if not members.size:
            return archive
        self.engine.archive_append_members(members)
        return np.concatenate([archive, self.engine.archive_get_points(len(archive), members.size)])

    def offspring(self, i, ret, length):
        return Offspring(self.tasks[i], [ret], [length])

    def evaluate(self, individuals, tslimit):
        return _evaluate(self.engine, [o.seeds for o in individuals], tslimit, self.rs)

    def next_parents(self, selected, had_parents):
        pass


def _ns_loop(log_dir, exp, k, prob, side, engine, rs, game, model, P, indices, max_iters):
    """GA-NS (the Deep-GA paper's novelty-search GA, Lehman and Stanley's novelty) behind maze_ns_main, dense_ns_main and atari_ns_main: the resume,
    the generations and the Novelty* rows, once.  side is a _BankNs or an _AtariNs, (k, prob) what _check_ns returned, (game, model, P) what the
    snapshot is held to (P None on the maze: its state carries no num_params), indices the number of admissible noise indices.  Returns what
    main returns.

    The reference has no GA-NS code (gpu_implementation/README.md leaves it for later), so every decision here is ours; the three drivers'
    docstrings say what each family adds:
      draws        maze_main's two whole-array draws first, then rs.random_sample(n) < archive_prob: this generation's archive mask; then
                   whatever the family's evaluation calls draw.
      scoring      ONE evaluation of the generation, then the family's pool novelty (k) where the evaluation left the behaviour
                   characterisations: each member against the archive and the other members of its generation.  The n doubles are all that
                   comes back.
      non-finite   a novelty that is not finite counts as 0.0 (nses_gpu's rule, nses_gpu.sanitized): the lowest there is, so a NaN policy is
                   never selected ahead of a finite one.
      order        descending novelty, then arrival index, by a stable host sort of the doubles (ga_select is float32 and would make
                   ties the doubles do not have).
      parents      the top T by novelty.  No reward elite enters the bank: every parent of the next generation is a child descriptor of
                   this one (the promote call never takes the kept form); generation 0's roots are built once.
      archive      after scoring, the masked members are appended in arrival order by one append_members call, device to device:
                   a generation is never scored against its own entries.
      reporting    the validation set is this generation's top V by reward (ga_select), without the [elite] + carry; elite, test episodes
                   and curr_solution_* follow ga.py's rules on that set.  The reward is never used for selection.
      genomes      Offspring objects exist for the union of the top T by novelty and the top V by reward: state.population holds the
                   former in novelty order, then the rest of the latter in reward order.
      snapshot     algo = 'ga_ns', game, model, the archive, k, archive_prob and the stream; a resume pushes the archive back and continues
                   bit for bit.  A resume from a 'ga', es_gpu or nses_gpu snapshot, or under another game, model, P, k or archive_prob,
                   raises and names both.
      T == 0       allowed: random search, with an archive that still fills.
    Tabular keys: maze_main's, plus NoveltyMean, NoveltyMax (after the non-finite rule), ArchiveSize and, for the bank families,
    BestDistanceToGoal = -max reward."""
    from .nses_gpu import sanitized                                 # nses_gpu imports this module's Schedule
    n, T, V = exp['population_size'], exp['selection_threshold'], exp['validation_threshold']
    all_tstart = time.time()
    side.clear()
    state = _resume(log_dir, ALGO_NS, rs, game or 'an Atari game', model, P)
    if state is None:
        state = TrainingState(exp)
        state.archive, state.stream = side.empty, None
    else:
        if (state.k, state.archive_prob) != (k, prob):
            raise ValueError("snapshot.pkl in {} holds k {}, archive_prob {!r}; this run is k {}, archive_prob {!r}".format(
                log_dir, state.k, state.archive_prob, k, prob))
        if len(state.archive):
            side.append(state.archive)
    state.game, state.model, state.algo, state.k, state.archive_prob = game, model, ALGO_NS, k, prob
    if P is not None:
        state.num_params = P
    if 'load_population' in exp:
        state.copy_population(exp['load_population'])
    parents = [o.seeds for o in state.population[:T]]               # the genomes of the parents: the top T by novelty, no elite carried
    if parents:
        side.build(parents)
    iters = 0
    while max_iters is None or iters < max_iters:
        iters += 1
        tstart_iteration = time.time()
        if state.timesteps_so_far >= exp['timesteps']:
            break
        assert (len(parents) == 0 and (state.it == 0 or T == 0)) or len(parents) == T
        power = state.sample(state.mutation_power)
        of, idx = _draw_generation(rs, n, len(parents), indices)
        archived = np.flatnonzero(rs.random_sample(n) < prob).astype(np.int32)
        rets, lens = side.generation(of, idx, power, parents, state.tslimit)
        novelty = sanitized(side.novelty_pool(k))                   # against the archive as it was before this generation, and the generation
        state.archive = side.append_members(archived, state.archive)   # ahead of the validation episodes: on Atari they overwrite the recorded states
        state.num_frames += int(lens.sum()) * side.frames
        state.it += 1
        rewards = np.asarray(rets, np.float64)
        by_novelty = np.argsort(-novelty, kind='stable')            # (-novelty, arrival index)
        by_reward = engine.ga_select(np.asarray(rets, np.float32), n)
        offspring = {}                                              # member index -> its Offspring
        for i in list(by_novelty[:T]) + list(by_reward[:V]):
            i = int(i)
            if i not in offspring:
                offspring[i] = side.offspring(i, float(rets[i]), int(lens[i]))
                offspring[i].novelty = float(novelty[i])
        selected = [offspring[int(i)] for i in by_novelty[:T]]
        validation_population = [offspring[int(i)] for i in by_reward[:V]]
        state.population = selected + [o for o in validation_population if not any(o is s for s in selected)]
        v = _validate_and_test(state, exp, validation_population, side.evaluate, int(lens.sum()))
        side.next_parents(selected, bool(parents))
        parents = [o.seeds for o in selected]
        dt = time.time() - tstart_iteration
        state.time_elapsed += dt
        _record_rows(state, power, rewards, T, v, dt, all_tstart)
        rows = [('NoveltyMean', float(np.mean(novelty))), ('NoveltyMax', float(np.max(novelty))), ('ArchiveSize', int(state.archive.shape[0]))]
        if side.goal_row:
            rows.append(('BestDistanceToGoal', -float(np.max(rewards))))
        for key, val in rows:
            tlogger.record_tabular(key, val)
        tlogger.dump_tabular()
        _end_generation(state, log_dir, lens, rs)
        if state.timesteps_so_far >= exp['timesteps']:
            break
    return float(state.curr_solution_test), {'val': float(state.curr_solution_val)}, state


def maze_ns_main(log_dir, engine=None, noise=None, seed=0, max_iters=None, **exp):
    """GA-NS on game 'maze' under 'SimpleClassifier': maze_main's loop with novelty as the fitness (_ns_loop, whose docstring holds the decisions).
    exp['novelty_search'] = {'k': 1 .. MAZE_NOVELTY_KMAX, 'archive_prob': 0 .. 1}.  Returns what maze_main returns.

    On the maze:
      draws        nothing beyond the loop's three: the episode is deterministic, no environment seed is drawn.
      scoring      one maze_ga_eval, then maze_novelty_pool(k) where k_maze_rollout left the final positions (csrc/maze_novelty.h, the pool
                   form); the masked members are appended by one maze_archive_append_members.
      parents      maze_ga_build for generation 0's roots, one maze_ga_promote of child descriptors after that.
      snapshot     game 'maze', model 'SimpleClassifier', no num_params; the archive is float32 [A][2], read back whole.
    num_frames counts steps, as in maze_main."""
    k, prob = _check_ns(exp, 'MAZE_NOVELTY_KMAX')
    engine, noise, rs = _open_maze_run(log_dir, engine, noise, seed, exp)
    return _ns_loop(log_dir, exp, k, prob, _BankNs(_MazeBank(engine)), engine, rs, 'maze', MAZE_MODEL, None, len(noise.noise) - engine.P + 1, max_iters)


def dense_ns_main(log_dir, engine=None, noise=None, seed=0, max_iters=None, **exp):
    """GA-NS over a dense policy of any small shape on the maze, the cart-pole or the acrobot (a DNE_KIND_DENSE engine): _ns_loop, its decisions
    and its tabular keys, on the dense bank (dense_ga_*) with novelty over final states (csrc/dense_novelty.h, the pool form).
    exp['novelty_search'] = {'k': 1 .. DENSE_NOVELTY_KMAX, 'archive_prob': 0 .. 1}.  Returns what main returns.  DESIGN.md section 17c.

    Called directly: main and dense_main raise NotImplementedError for exp['novelty_search'] on a dense run.  The engine is opened and checked
    as dense_main does it (same routing, same refusals), the init scale is policies.dense_scale_by of the shape.  What differs from maze_ns_main:
      draws        the two whole-array draws, then rs.random_sample(n) < archive_prob; on the cart-pole the generation's environment seeds
                   follow (drawn by the evaluation, as every evaluation call of dense_main draws them), and each validation and test call draws
                   its own.  On the maze nothing more is drawn: a (16, 16) relu engine on the maze consumes maze_ns_main's stream draw for draw.
      BC           section 17b's: one episode's final state record cast to D floats (maze (x, y), cart-pole (x, x_dot, theta, theta_dot), acrobot (theta1, theta2, omega1, omega2)).  On
                   the cart-pole it is the ONE episode the generation ran under its drawn seed; no mean BC over several episodes.
      scoring      one dense_ga_eval, then dense_novelty_pool(k) on the BCs of that evaluation, on the device; the masked members are appended
                   afterwards by one dense_archive_append_members.
      limits       dense_main's: a generation and the validation episodes under state.tslimit, at most the environment's own limit; the test
                   episodes at the environment's own limit.  num_frames counts steps.
      snapshot     num_params = P as well, the archive [A][D]; a resume pushes it back with dense_archive_append."""
    k, prob = _check_ns(exp, 'DENSE_NOVELTY_KMAX')
    engine, noise, game, model = _open_dense_run('dense_ns_main', log_dir, engine, noise, exp)
    rs = np.random.RandomState(seed)
    return _ns_loop(log_dir, exp, k, prob, _BankNs(_DenseBank(engine, rs)), engine, rs, game, model, engine.P, len(noise.noise) - engine.P + 1, max_iters)


def atari_ns_main(log_dir, engine=None, noise=None, seed=0, max_iters=None, **exp):
    """GA-NS on an Atari game under `Model` / `LargeModel`: main's Atari evaluation (the genome store behind ga_eval_powers, HipModel) in
    _ns_loop, with its decisions and tabular keys (without BestDistanceToGoal), novelty over the members' final 128-byte RAM states
    (GAAtariPolicy.rollout's behaviour characterisation, policies.py:510) scored on the device (csrc/ram_novelty.h).
    exp['novelty_search'] = {'k': 1 .. RAM_NOVELTY_KMAX, 'archive_prob': 0 .. 1}.  Returns what main returns.

    Called directly: main raises NotImplementedError for exp['novelty_search'] under an Atari game.  What differs from maze_ns_main:
      engine       a caller's engine must be of the model's kind (KIND_GA for 'Model', KIND_GA_LARGE for 'LargeModel') and created with
                   record_bc (ValueError otherwise); without one, an engine with record_bc and max_members = population_size is opened.  The
                   population must fit engine.max_members (ValueError): the whole generation is ONE ga_eval_powers, because the last
                   evaluation is the pool.
      draws        the two whole-array draws, then rs.random_sample(n) < archive_prob, then the generation's n environment seeds (drawn by
                   the evaluation, as every evaluation call of main draws them); each validation and test call draws its own.
      genomes      every member's genome is written out (ga_eval_powers takes genomes; the store keeps the parents' vectors cached).
      scoring      one ga_eval_powers, then ram_novelty_pool(k) on the final RAM states where the evaluation left them; the masked members
                   are appended afterwards by one archive_append_members, before the validation episodes overwrite the recorded states.
      limits       main's: a generation and the validation episodes under state.tslimit, the test episodes under the environment's own
                   limit.  num_frames counts 4 frames a step.
      snapshot     num_params = P as well, the archive uint8 [A][128] (read back through archive_get_points, the appended entries only);
                   a resume pushes it back with archive_append_points."""
    k, prob = _check_ns(exp, 'RAM_NOVELTY_KMAX')
    n, asked = exp['population_size'], exp.get('model', 'Model')
    if asked not in MODEL_KINDS or exp.get('game') == 'maze' or _is_dense_run(None, exp):
        raise NotImplementedError("model {!r} on game {!r}: atari_ns_main runs {} on an Atari game".format(
            asked, exp.get('game'), ' and '.join(repr(m) for m in sorted(MODEL_KINDS))))
    if engine is None:
        engine = _lib.Engine(MODEL_KINDS[asked], 18, max_members=n, record_bc=True)
    elif engine.kind != MODEL_KINDS[asked]:
        raise ValueError("model {!r} asked for (engine kind {}), the engine passed in is of kind {}".format(asked, MODEL_KINDS[asked], engine.kind))
    if not getattr(engine, 'record_bc', False):
        raise ValueError("atari_ns_main needs an engine created with record_bc: the final RAM states are the behaviour characterisations")
    if n > engine.max_members:
        raise ValueError("population_size {} exceeds the engine's max_members {}: a GA-NS generation is one evaluation, its members are the pool".format(
            n, engine.max_members))
    tlogger.start(log_dir)
    noise = noise if noise is not None else SharedNoiseTable()
    noise.attach(engine)
    engine.ga_set_init_scale(model_scale_by(engine.n_actions, engine.kind))     # as HipModel sets it for main
    rs = np.random.RandomState(seed)
    return _ns_loop(log_dir, exp, k, prob, _AtariNs(engine, rs), engine, rs, exp.get('game'), asked, engine.P, len(noise.noise) - engine.P + 1, max_iters)

