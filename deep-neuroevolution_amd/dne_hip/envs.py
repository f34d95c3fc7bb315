"""The hard maze, the cart-pole, the pendulum and the acrobot as batched environments of their own: the surface of the GPU tree's
gym_tensorflow/tf_env.py:27-124 (reset / step / observation / final_state apart from the model) without TensorFlow, over the engine's
step-at-a-time batch (csrc/step_env.h, dne_stepenv_*).  One object = the first batch_size environments of one engine; every value it returns
is the one the whole-episode kernels compute, bit for bit, so a policy the kernels do not contain -- a LinearClassifier, a wider net, a
hand-written controller -- can be run against the same environments:

    env = envs.make('gym.CartPole-v1', 64)
    returns, lengths = envs.rollout(env, lambda obs: (obs[:, 2] > 0).astype(np.int32))

The reference's reset is unseeded; here seeds=None draws uint32 seeds from a RandomState(seed) the object holds."""
import numpy as np

from . import _lib
from .maze_run import maze_file

MAZE_GAME, CARTPOLE_GAME, PENDULUM_GAME, ACROBOT_GAME = 'maze', 'gym.CartPole-v1', 'Pendulum-v0', 'gym.Acrobot-v1'


class HipStepEnv:
    """what the four classes share; a subclass names its kind, game and env_default_timestep_cutoff (n_actions: of a discrete action space)"""
    kind = None
    n_actions = 2
    game = None
    env_default_timestep_cutoff = None

    def __init__(self, batch_size, engine=None, seed=0, hidden=None, nonlin='relu'):
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("{}: a batch of {} environments".format(self.game, batch_size))
        if engine is not None and getattr(engine, 'env_kind', engine.kind) != self.kind:   # (a KIND_DENSE engine steps the environment it was created on)
            raise ValueError("game {!r} asked for, the engine passed in is of kind {} (kind {} runs it)".format(self.game, engine.kind, self.kind))
        if engine is not None and engine.max_members < batch_size:
            raise ValueError("game {!r}: a batch of {} environments, the engine passed in holds {}".format(self.game, batch_size, engine.max_members))
        self._own = engine is None
        self.engine = (self._open(batch_size) if hidden is None else self._open_dense(batch_size, hidden, nonlin)) if engine is None else engine
        self.batch_size = batch_size
        self._obs_w, self._act_w, self._state_w, self._int_act = _lib.stepenv_dims(self.kind)
        self.np_random = np.random.RandomState(seed)

    def _open(self, batch_size):
        return _lib.Engine(self.kind, 2, max_members=batch_size)

    def _open_dense(self, batch_size, hidden, nonlin):
        """an engine whose policy is a dense stack of the caller's shape (hidden: the tuple of widths, () a LinearClassifier) on this environment"""
        return _lib.Engine(_lib.KIND_DENSE, 1 if self.kind == _lib.KIND_PENDULUM else self.n_actions, max_members=batch_size, env=self.kind, hidden=tuple(hidden), nonlin=nonlin)

    # ---- tf_env.py's properties
    @property
    def observation_space(self):
        return (self._obs_w,)

    @property
    def action_space(self):
        """the number of actions (discrete) or the action's width (continuous)"""
        return self.n_actions if self._int_act else self._act_w

    @property
    def discrete_action(self):
        return self._int_act

    @property
    def unwrapped(self):
        return self

    def _indices(self, indices):
        return np.arange(self.batch_size, dtype=np.int32) if indices is None else np.ascontiguousarray(indices, np.int32).reshape(-1)

    # ---- tf_env.py's calls
    def reset(self, indices=None, max_frames=None, seeds=None):
        """the named environments restart; max_frames=None (or <= 0): env_default_timestep_cutoff.  seeds uint32 [n], None: drawn from np_random"""
        idx = self._indices(indices)
        if seeds is None:
            seeds = self.np_random.randint(0, 2 ** 32, size=idx.size, dtype=np.uint64).astype(np.uint32)
        self.engine.stepenv_reset(idx, seeds, 0 if max_frames is None else int(max_frames))

    def step(self, action, indices=None):
        """one step of the named environments -> (reward float32 [n], done bool [n]); a done environment stays as it is and earns 0"""
        return self.engine.stepenv_step(action, self._indices(indices))

    def observation(self, indices=None):
        """float32 [n][obs]: what a policy acts on next"""
        return self.engine.stepenv_observation(self._indices(indices))

    def final_state(self, indices=None):
        """float32 [n][2]: zeros, as PythonEnv.final_state (tf_env.py:71-73); the maze returns its (x, y)"""
        return np.zeros((self._indices(indices).size, 2), np.float32)

    def state(self, indices=None):
        """(state float64 [n][S], steps int32 [n], done bool [n])"""
        return self.engine.stepenv_state(self._indices(indices))

    def set_state(self, state, steps=None, indices=None, max_frames=None):
        """put the named environments into given states (done cleared, the observation recomputed)"""
        self.engine.stepenv_set_state(state, steps, self._indices(indices), 0 if max_frames is None else int(max_frames))

    def close(self):
        if self._own and self.engine is not None:
            self.engine.close()
        self.engine = None


class HipMazeEnv(HipStepEnv):
    """the hard maze (gym_tensorflow/maze/): 11 observations, two raw outputs as the action, 400 steps, the reward on the last of them"""
    kind, game, env_default_timestep_cutoff = _lib.KIND_MAZE, MAZE_GAME, _lib.MAZE_STEPS

    def __init__(self, batch_size, engine=None, seed=0, maze_file=None, hidden=None, nonlin='relu'):
        self._maze_file = maze_file
        super().__init__(batch_size, engine, seed, hidden, nonlin)
        if self._own or maze_file is not None:
            self.engine.maze_set_walls(*_lib.load_maze(self._path()))

    def _path(self):
        return maze_file({} if self._maze_file is None else {'maze_file': self._maze_file})

    def final_state(self, indices=None):
        return self.state(indices)[0][:, :2].astype(np.float32)


class HipCartPoleEnv(HipStepEnv):
    """gym.CartPole-v1: four observations, actions 0 / 1, at most 500 steps, reward 1 per step"""
    kind, game, env_default_timestep_cutoff = _lib.KIND_CARTPOLE, CARTPOLE_GAME, _lib.CARTPOLE_STEPS


class HipPendulumEnv(HipStepEnv):
    """the torque-limited pendulum swing-up: three raw observations (cos, sin, speed), one torque in [-2, 2] (clipped by the step), 200 steps"""
    kind, game, env_default_timestep_cutoff = _lib.KIND_PENDULUM, PENDULUM_GAME, _lib.PENDULUM_STEPS

    def _open(self, batch_size):
        # the engine's own policy (MujocoPolicy, the narrowest) is not used by the environments; the kind needs a shape to be created
        return _lib.Engine(self.kind, 1, max_members=batch_size, hidden=64)


class HipAcrobotEnv(HipStepEnv):
    """gym.Acrobot-v1 (csrc/acrobot.h): six observations (cos, sin of both angles, both velocities), actions 0 / 1 / 2 (torque -1 / 0 / +1), reward
    -1 a step and 0 on the step that swings the free end above the line, at most 500 steps.  There is no native engine kind: the engine is a
    KIND_DENSE one created on the environment (hidden=() unless given), whose policy envs.run puts behind the batch"""
    kind, game, env_default_timestep_cutoff, n_actions = _lib.ENV_ACROBOT, ACROBOT_GAME, _lib.ACROBOT_STEPS, _lib.ACROBOT_ACTIONS

    def _open(self, batch_size):
        return self._open_dense(batch_size, (), 'relu')


_GAMES = {MAZE_GAME: HipMazeEnv, CARTPOLE_GAME: HipCartPoleEnv, PENDULUM_GAME: HipPendulumEnv, ACROBOT_GAME: HipAcrobotEnv}


def make(game, batch_size, engine=None, **kw):
    """gym_tensorflow.make for the four games: 'maze' (maze_file=... as the maze drivers take it), 'gym.CartPole-v1', 'Pendulum-v0',
    'gym.Acrobot-v1' (always on a KIND_DENSE engine: the environment has no kind of its own).  engine:
    an Engine of the game's kind with max_members >= batch_size (None: one is made and closed with the environment); seed=... starts np_random.
    hidden=(...) (and nonlin='relu' or 'tanh'): the engine made is a KIND_DENSE one whose policy is a dense stack of those hidden widths on the
    game's environment (() is a LinearClassifier), so that run() below keeps whole episodes on the device; an engine of that kind may be passed in too"""
    if game not in _GAMES:
        raise NotImplementedError("game {!r}: the step-at-a-time environments are {}".format(game, ", ".join(repr(g) for g in _GAMES)))
    return _GAMES[game](batch_size, engine=engine, **kw)


def rollout(env, act, seeds=None, max_frames=None):
    """One episode of every environment of the batch: reset, then act(obs float32 [n][obs]) -> actions and a step of the whole batch until every
    member is done (a done member is stepped on at reward 0).  Returns (returns float32 [n], lengths int32 [n]).  Rewards are added per member
    in float64, in step order, and cast once: the whole-episode kernels' own accumulation."""
    env.reset(max_frames=max_frames, seeds=seeds)
    n = env.batch_size
    total, lengths, done = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, bool)
    while not done.all():
        live = ~done
        reward, done = env.step(act(env.observation()))
        total += reward.astype(np.float64)
        lengths += live
    return total.astype(np.float32), lengths


def run(env, members=None, max_steps=None, seeds=None, max_frames=None):
    """rollout's device counterpart on a KIND_DENSE engine: reset, then the policy of the engine's members behind the environments
    (members[i] under environment i; None: member i) in stepenv_run launches of max_steps rounds each (None: one launch to the end) until every
    environment is done.  Returns (returns float32 [n], lengths int32 [n]) with rollout's contract when the episodes finish in one launch; over
    several launches each launch's float64 sum is cast once and the casts are added in float64."""
    env.reset(max_frames=max_frames, seeds=seeds)
    n = env.batch_size
    if members is not None:
        members = np.ascontiguousarray(members, np.int32).reshape(-1)
    rounds = env.env_default_timestep_cutoff if max_steps is None else int(max_steps)
    total, lengths, done = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, bool)
    while not done.all():
        reward, steps, done = env.engine.stepenv_run(rounds, env._indices(None), members)
        total += reward.astype(np.float64)
        lengths += steps
    return total.astype(np.float32), lengths
