"""Host-side mirror of es_distributed/policies.py for the Atari policies, backed by the HIP engine.

Keeps the reference's Policy surface (policies.py:15-113, 305-513): num_params, set_trainable_flat /
get_trainable_flat, set_ref_batch, needs_ob_stat / needs_ref_batch, reinitialize, act, rollout, save / Load.
The network itself never exists on the host: parameters are a flat float32 vector in the creation order
of the reference's trainable variables (flat_layout below), the forward runs in libdne_hip.so.
"""
import pickle
from collections import OrderedDict

import numpy as np

from . import _lib


def flat_layout(kind, nact):
    """Offsets of each trainable variable in the flat vector (policies.py:21-24, tf_util.py:224-246).
    ESAtariPolicy: tf.contrib.layers order (weights, biases, BN beta, BN gamma per layer), policies.py:319-330.
    GAAtariPolicy: U.conv / U.dense order (w, b), policies.py:449-459 via tf_util.py:133-162.
    ModelVirtualBN (the GPU tree's ES model, models/batchnorm.py:52-123): creation order (base.py:35-44, 166-178) -- conv / fc without
    bias, each followed by its BatchNorm/b (the shift after normalisation; BN mean / var are not in the vector), then out/w, out/b."""
    spec = OrderedDict()
    o = 0

    def add(name, shape):
        nonlocal o
        spec[name] = (o, tuple(shape))
        o += int(np.prod(shape))

    if kind == _lib.KIND_ES:
        add("conv1/weights", (8, 8, 4, 16)); add("conv1/biases", (16,)); add("BatchNorm/beta", (16,)); add("BatchNorm/gamma", (16,))
        add("conv2/weights", (4, 4, 16, 32)); add("conv2/biases", (32,)); add("BatchNorm_1/beta", (32,)); add("BatchNorm_1/gamma", (32,))
        add("fc/weights", (3872, 256)); add("fc/biases", (256,)); add("BatchNorm_2/beta", (256,)); add("BatchNorm_2/gamma", (256,))
        add("out/weights", (256, nact)); add("out/biases", (nact,))
    elif kind == _lib.KIND_ES_VBN:
        add("layer1/conv1/w", (8, 8, 4, 16)); add("layer1/BatchNorm/b", (1, 1, 1, 16))
        add("layer2/conv2/w", (4, 4, 16, 32)); add("layer2/BatchNorm/b", (1, 1, 1, 32))
        add("layer3/fc/w", (3872, 256)); add("layer3/BatchNorm/b", (1, 256))
        add("layer4/out/w", (256, nact)); add("layer4/out/b", (1, nact))
    elif kind == _lib.KIND_MAZE:       # the GPU tree's SimpleClassifier on the maze's 11 inputs, models/simple.py:29-35 (nact = 2: the raw outputs are the action)
        add("fc1/w", (11, 16)); add("fc1/b", (1, 16))
        add("fc2/w", (16, 16)); add("fc2/b", (1, 16))
        add("out/w", (16, nact)); add("out/b", (1, nact))
    elif kind == _lib.KIND_CARTPOLE:   # the same SimpleClassifier on CartPole-v1's 4 inputs (nact = 2: the first maximum of the outputs is the action)
        add("fc1/w", (4, 16)); add("fc1/b", (1, 16))
        add("fc2/w", (16, 16)); add("fc2/b", (1, 16))
        add("out/w", (16, nact)); add("out/b", (1, nact))
    elif kind == _lib.KIND_GA_LARGE:   # the GPU tree's LargeModel, gpu_implementation/neuroevolution/models/dqn.py:39-47 (creation order, base.py:35-41)
        add("conv1/w", (8, 8, 4, 32)); add("conv1/b", (1, 1, 1, 32))
        add("conv2/w", (4, 4, 32, 64)); add("conv2/b", (1, 1, 1, 64))
        add("conv3/w", (3, 3, 64, 64)); add("conv3/b", (1, 1, 1, 64))
        add("fc/w", (7744, 512)); add("fc/b", (1, 512))
        add("out/w", (512, nact)); add("out/b", (1, nact))
    else:
        add("conv1/w", (8, 8, 4, 16)); add("conv1/b", (1, 1, 1, 16))
        add("conv2/w", (4, 4, 16, 32)); add("conv2/b", (1, 1, 1, 32))
        add("fc/w", (3872, 256)); add("fc/b", (256,))
        add("out/w", (256, nact)); add("out/b", (nact,))
    return spec, o


def vbn_scale_by(nact):
    """scale_by of ModelVirtualBN (models/dqn.py:25-27 via batchnorm.py:52, base.py:166-178): each w gets std / sqrt(prod(shape[:-1]))
    with std 1.0 -- the out layer included (batchnorm.py:105 passes no std=0.1, unlike Model) --, each b 0.  fp32, in flat_layout order:
    theta_0 = noise.get(idx, P) * scale_by (base.py:123-141)."""
    spec, P = flat_layout(_lib.KIND_ES_VBN, nact)
    sb = np.zeros(P, np.float32)
    for name, (off, shape) in spec.items():
        if name.endswith('/w'):
            sb[off:off + int(np.prod(shape))] = np.float32(1.0 / np.sqrt(np.prod(shape[:-1])))
    return sb


def simple_scale_by(kind=_lib.KIND_MAZE):
    """scale_by of SimpleClassifier on the hard maze (models/simple.py:29-35 over dqn.Model, dqn.py:25-27): std / sqrt(prod(shape[:-1])) for each
    w -- 1/sqrt(11), 1/4 and (std = 0.1 for the out layer) 0.1/4 --, 0 for each b.  fp32, in flat order; theta_0 = noise.get(idx, 498) * scale_by.
    kind = KIND_CARTPOLE: the same model on 4 inputs -- 1/sqrt(4), 1/4, 0.1/4 --, 386 values."""
    if kind not in (_lib.KIND_MAZE, _lib.KIND_CARTPOLE):
        raise ValueError("simple_scale_by: kind {} does not run SimpleClassifier (KIND_MAZE {} and KIND_CARTPOLE {} do)".format(
            kind, _lib.KIND_MAZE, _lib.KIND_CARTPOLE))
    spec, P = flat_layout(kind, 2)
    sb = np.zeros(P, np.float32)
    for name, (off, shape) in spec.items():
        if name.endswith('/w'):
            std = 0.1 if name.startswith('out') else 1.0
            sb[off:off + int(np.prod(shape))] = np.float32(std / np.sqrt(np.prod(shape[:-1])))
    return sb


def dense_scale_by(env_kind, hidden, n_out):
    """scale_by of a dense stack on a step environment (a KIND_DENSE engine's flat order: per layer w [in][out], then b [out]):
    Model.create_weight_variable's std / sqrt(prod(shape[:-1])) for each w, 0 for each b.  std is 1.0, and 0.1 on the last layer of a stack
    with hidden layers (models/simple.py:34); LinearClassifier's single layer (hidden = ()) keeps 1.0 (simple.py:26).  For (16, 16) on the
    maze or the cart-pole it is simple_scale_by."""
    hidden = tuple(int(w) for w in hidden)
    dims = (_lib.stepenv_dims(env_kind)[0],) + hidden + (int(n_out),)
    parts = []
    for l in range(len(dims) - 1):
        std = 0.1 if hidden and l == len(dims) - 2 else 1.0
        parts.append(np.full(dims[l] * dims[l + 1], np.float32(std / np.sqrt(dims[l])), np.float32))
        parts.append(np.zeros(dims[l + 1], np.float32))
    return np.concatenate(parts)


def xavier_flat(nact, seed=0):
    """Initial ESAtariPolicy parameters: tf.contrib.layers defaults (xavier-uniform weights, zero biases,
    BN beta 0 / gamma 1) drawn from RandomState(seed) -- TF's own initialiser is unseeded."""
    spec, P = flat_layout(_lib.KIND_ES, nact)
    rs = np.random.RandomState(seed)
    th = np.zeros(P, np.float32)
    for name, (off, shape) in spec.items():
        n = int(np.prod(shape))
        if name.endswith("weights"):
            rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
            lim = np.sqrt(6.0 / (shape[-2] * rf + shape[-1] * rf))
            th[off:off + n] = rs.uniform(-lim, lim, n).astype(np.float32)
        elif name.endswith("gamma"):
            th[off:off + n] = 1.0
    return th


class _Space:
    def __init__(self, shape=None, n=None):
        self.shape, self.n = shape, n


class HipAtariEnv:
    """The engine's batched environment seen through the gym-style surface the reference drivers use
    (es.py:131-133: gym.make + wrap_deepmind).  One instance = env slot 0 of an Engine."""
    observation_space = _Space(shape=_lib.OB_SHAPE)

    def __init__(self, engine, seed=0):
        self.engine = engine
        self.action_space = _Space(n=engine.n_actions)
        self._episode = 0
        self._seed = int(seed)
        self.np_random = np.random.RandomState(seed)

    def seed(self, seed):
        self._seed, self._episode = int(seed), 0
        self.np_random = np.random.RandomState(seed)

    def next_episode_seed(self):
        s = (self._seed + self._episode) & 0xFFFFFFFF
        self._episode += 1
        return s

    def reset(self):
        self.engine.env_reset(np.array([self.next_episode_seed()], np.uint32))
        return self._ob()

    def step(self, action):
        rew, done = self.engine.env_step(np.array([action], np.int32))
        return self._ob(), float(rew[0]), bool(done[0]), {}

    def _ob(self):  # ScaledFloatFrame: float32(u8) / 255.0  (atari_wrappers.py:183-186)
        return self.engine.env_observation(1)[0].astype(np.float32) / np.float32(255.0)

    def _get_ram(self):
        return self.engine.env_ram(1)[0]

    @property
    def unwrapped(self):
        return self


class Policy:
    kind = None

    def __init__(self, ob_space, ac_space, engine=None, **kwargs):
        self.args, self.kwargs = (ob_space, ac_space), kwargs
        self.ob_space_shape = tuple(ob_space.shape)
        self.ac_space = ac_space
        self.num_actions = ac_space.n
        self.spec, self.num_params = flat_layout(self.kind, self.num_actions)
        self.engine = engine
        self._flat = np.zeros(self.num_params, np.float32)
        assert self.num_params == _lib.num_params(self.kind, self.num_actions)

    # policies.py:99-103
    def set_trainable_flat(self, x):
        x = np.asarray(x, np.float32)
        assert x.shape == (self.num_params,)
        self._flat = x.copy()
        if self.engine is not None:
            self.engine.set_theta(self._flat, slot=0)

    def get_trainable_flat(self):
        if self.engine is not None:
            self._flat = self.engine.get_theta(0)
        return self._flat.copy()

    @property
    def needs_ob_stat(self):
        return False

    def act(self, ob, random_stream=None):
        """policies.py:374-375 / 469-470: argmax action for a batch of float observations in [0, 1]."""
        obs = np.asarray(ob[0] if isinstance(ob, (list, tuple)) else ob, np.float32)
        u8 = np.rint(obs * 255.0).astype(np.uint8).reshape((-1,) + _lib.OB_SHAPE)
        n = u8.shape[0]
        e = self.engine
        e.env_set_observation(u8)
        e.set_members(np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.float32))
        if self.kind == _lib.KIND_ES:
            e.ref_pass(n)
        return e.act(n)[0].astype(np.int64)

    def rollout(self, env, *, render=False, timestep_limit=None, save_obs=False, random_stream=None,
                worker_stats=None, policy_seed=None):
        """policies.py:378-429 / 473-513: one episode of the current flat parameters.  Returns
        (rews float32[T], T, novelty_vector) like the reference (ES: RAM per step, GA: final RAM)."""
        e = self.engine
        limit = _lib.ENV_MAX_EPISODE_STEPS if timestep_limit is None else min(timestep_limit, _lib.ENV_MAX_EPISODE_STEPS)
        if policy_seed:
            env.seed(policy_seed)
        seed = env.next_episode_seed()
        e.set_members(np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.float32))
        # a single episode needs per-step rewards: drive it step by step through the env ABI
        e.env_reset(np.array([seed], np.uint32))
        if self.kind == _lib.KIND_ES:
            e.ref_pass(1)
        rews, rams, obs = [], [], []
        for _ in range(limit):
            if save_obs:
                obs.append(e.env_observation(1)[0].astype(np.float32) / np.float32(255.0))
            a = e.act(1)[0]
            rew, done = e.env_step(a)
            rews.append(rew[0])
            if self.kind == _lib.KIND_ES:
                rams.append(e.env_ram(1)[0])
            if done[0]:
                break
        nov = np.array(rams) if self.kind == _lib.KIND_ES else e.env_ram(1)[0]
        rews = np.array(rews, dtype=np.float32)
        if save_obs:
            return rews, len(rews), np.array(obs), nov
        return rews, len(rews), nov

    # ---- snapshots, policies.py:49-67
    def variable_arrays(self):
        """{TF variable name: array} for every variable the reference's Policy.save writes (policies.py:52-53:
        `for v in self.all_variables: f[v.name] = v.eval()`), e.g. 'ESAtariPolicy/conv1/weights:0'."""
        flat = self.get_trainable_flat()
        scope = type(self).__name__
        out = OrderedDict()
        for name, (off, shape) in self.spec.items():
            out['%s/%s:0' % (scope, name)] = flat[off:off + int(np.prod(shape))].reshape(shape).copy()
        out.update(self.extra_variable_arrays(scope))
        return out

    def extra_variable_arrays(self, scope):
        return {}

    def save(self, filename):
        """policies.py:49-57.  '.h5': the reference's HDF5 layout -- a float32 dataset per TF variable name, root attributes
        'name' and 'args_and_kwargs' -- written through h5py when it is installed, else through libhdf5 directly
        (h5lite.py; this image has the C library but not h5py).  Any other name: the same arrays, names and attributes in
        a numpy container, which tools/npz_to_h5.py turns into the .h5 (snapshot_extension() picks what the drivers use)."""
        arrays = self.variable_arrays()
        blob = self._spaces_blob() if filename.endswith('.h5') else \
            pickle.dumps((((tuple(self.ob_space_shape), self.num_actions)), self.kwargs), protocol=-1)
        if filename.endswith('.h5'):
            try:
                import h5py
            except ImportError:
                h5py = None
            if h5py is not None:
                with h5py.File(filename, 'w', libver='latest') as f:
                    for k, v in arrays.items():
                        f[k] = v
                    f.attrs['name'] = type(self).__name__
                    f.attrs['args_and_kwargs'] = np.void(blob)
                return
            from . import h5lite
            if not h5lite.available():
                raise RuntimeError("writing '.h5' snapshots needs h5py or libhdf5 (neither found; DNE_HDF5_LIB names the "
                                   "library): save to '.npz' and run tools/npz_to_h5.py where h5py exists")
            h5lite.write_snapshot(filename, arrays, type(self).__name__, blob)
            return
        np.savez(filename, __name__=type(self).__name__, __args_and_kwargs__=np.void(blob),
                 __variables__=np.array(list(arrays.keys())), **{'var%03d' % i: v for i, v in enumerate(arrays.values())})

    def _spaces_blob(self):
        return _dumps_spaces(tuple(self.ob_space_shape), self.num_actions, self.kwargs)

    @staticmethod
    def _read_snapshot(filename):
        """-> (class name, (ob_shape, nact), kwargs, {variable name: array})"""
        if filename.endswith('.h5'):
            try:
                import h5py
            except ImportError:
                h5py = None
            if h5py is not None:
                with h5py.File(filename, 'r') as f:
                    blob = f.attrs['args_and_kwargs'].tobytes()
                    arrays = {}
                    f.visititems(lambda n, o: arrays.__setitem__(n, o[...]) if isinstance(o, h5py.Dataset) else None)
                    name = f.attrs['name']
            else:
                from . import h5lite
                name, blob, arrays = h5lite.read_snapshot(filename)
            args, kwargs = _loads_spaces(blob)
            ob, ac = args[0], args[1]     # the reference pickles gym spaces; ours are (shape, n)
            ob_shape = getattr(ob, 'shape', None) or (ob.low.shape if hasattr(ob, 'low') else ob)
            nact = getattr(ac, 'n', None) or (ac.low.shape[0] if hasattr(ac, 'low') else ac)
            return name, (tuple(ob_shape), int(nact)), kwargs, arrays
        with np.load(filename, allow_pickle=False) as f:
            (ob_shape, nact), kwargs = pickle.loads(f['__args_and_kwargs__'].tobytes())
            names = [str(n) for n in f['__variables__']]
            arrays = {n: f['var%03d' % i] for i, n in enumerate(names)}
            return str(f['__name__']), (tuple(ob_shape), int(nact)), kwargs, arrays

    @classmethod
    def Load(cls, filename, engine=None, extra_kwargs=None):
        """policies.py:59-67"""
        _, (ob_shape, nact), kwargs, arrays = cls._read_snapshot(filename)
        if extra_kwargs:
            kwargs.update(extra_kwargs)
        pol = cls(_Space(shape=ob_shape), _Space(n=nact), engine=engine, **kwargs)
        pol._set_from_arrays(arrays, exact=True)
        return pol

    def _set_from_arrays(self, arrays, exact):
        scope = type(self).__name__
        flat = self.get_trainable_flat() if not exact else np.zeros(self.num_params, np.float32)
        for name, (off, shape) in self.spec.items():
            a = np.asarray(arrays['%s/%s:0' % (scope, name)], np.float32)
            if exact:
                assert a.shape == shape, (name, a.shape, shape)
            else:   # policies.py:355-369: the loaded arrays may be smaller; they fill the leading sub-array
                assert a.ndim == len(shape) and all(x >= y for x, y in zip(shape, a.shape)), \
                    'This policy must have more weights than the policy to load'
            view = flat[off:off + int(np.prod(shape))].reshape(shape)
            view[tuple(slice(0, n) for n in a.shape)] = a
        self.set_trainable_flat(flat)

    def initialize_from(self, filename):
        """policies.py:345-372: weights from another policy of the same architecture (variable names), whose arrays may
        be smaller than this policy's."""
        _, _, _, arrays = self._read_snapshot(filename)
        mine = set(self.variable_arrays().keys())
        assert mine == set(arrays.keys()), 'Variable names do not match'
        self._set_from_arrays(arrays, exact=False)


class ESAtariPolicy(Policy):
    """policies.py:305-429: conv8s4x16 -> BN -> conv4s2x32 -> BN -> fc256 -> BN -> out, argmax; virtual batch norm."""
    kind = _lib.KIND_ES

    def set_ref_batch(self, ref_batch):  # policies.py:332-335
        ref = np.asarray(ref_batch)
        if ref.dtype != np.uint8:       # observations are exact multiples of 1/255 (atari_wrappers.py:183-186)
            ref = np.rint(ref.astype(np.float32) * 255.0).astype(np.uint8)
        self.ref_batch = ref
        if self.engine is not None:
            self.engine.set_ref_batch(ref)

    @property
    def needs_ref_batch(self):
        return True

    def reinitialize(self):
        raise NotImplementedError("ESAtariPolicy has no reinitialize ops in the reference (layers.* variables)")

    def initialize(self, seed=0):
        self.set_trainable_flat(xavier_flat(self.num_actions, seed))

    def extra_variable_arrays(self, scope):
        """BatchNorm*/moving_mean, moving_variance (policies.py:322-328: batch_norm(decay=0., updates_collections=None)
        overwrites them with the batch moments of every is_training pass, i.e. of the reference batch).  The engine
        computes those moments in its reference pass for the unperturbed theta; without an engine or a reference
        batch they are TF's initial values (zeros / ones)."""
        n = {'BatchNorm': 16, 'BatchNorm_1': 32, 'BatchNorm_2': 256}
        mom = None
        if self.engine is not None and getattr(self, 'ref_batch', None) is not None and hasattr(self.engine, 'get_bn_moments'):
            e = self.engine
            e.set_members(np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.float32))
            e.ref_pass(1)
            mom = e.get_bn_moments(1)[0]
        out, off = OrderedDict(), 0
        for bn, c in n.items():
            out['%s/%s/moving_mean:0' % (scope, bn)] = mom[off:off + c].copy() if mom is not None else np.zeros(c, np.float32)
            out['%s/%s/moving_variance:0' % (scope, bn)] = mom[off + c:off + 2 * c].copy() if mom is not None else np.ones(c, np.float32)
            off += 2 * c
        return out


class GAAtariPolicy(Policy):
    """policies.py:433-513: same trunk without batch norm, U.conv/U.dense with column-normalising reinitialize."""
    kind = _lib.KIND_GA

    def __init__(self, ob_space, ac_space, nonlin_type="relu", ac_init_std=0.1, engine=None):
        if nonlin_type != "relu":
            raise NotImplementedError("the HIP engine implements nonlin_type='relu' (configurations/frostbite_ga.json)")
        if ac_init_std != 0.1:
            raise NotImplementedError("ac_init_std is fixed at the reference default 0.1 (policies.py:434)")
        super().__init__(ob_space, ac_space, engine=engine, nonlin_type=nonlin_type, ac_init_std=ac_init_std)

    @property
    def needs_ref_batch(self):
        return False

    def set_from_seeds(self, seeds, noise_stdev):
        """ga.py:256-264 / 151-158: theta = normc(noise[s0]) + noise_stdev * sum noise[s_k], built on device."""
        self._flat = self.engine.ga_rebuild(0, np.asarray(seeds, np.int64), noise_stdev)
        return self._flat


# ---------------------------------------------------------------------------------------------- MujocoPolicy on the pendulum
PENDULUM_ENV_ID = 'Pendulum-v0'


class PendulumEnv:
    """The spaces of the torque-limited pendulum swing-up (csrc/pendulum.h) behind the gym-style surface es.setup reads: a Box observation of
    shape (3,), a Box action of shape (1,) with the finite bounds MujocoPolicy asserts (policies.py:130-132), 200 steps.  Episodes run inside
    the engine (or its host twin); this object only hands out their reset seeds."""
    max_episode_steps = _lib.PENDULUM_STEPS

    def __init__(self, engine=None, seed=0):
        self.engine = engine
        self.observation_space = _Space(shape=(_lib.PENDULUM_OBS,))
        self.action_space = _Space(shape=(1,))
        self.action_space.low, self.action_space.high = np.array([-2.0], np.float32), np.array([2.0], np.float32)
        self._seed, self._episode = int(seed), 0

    def seed(self, seed):
        self._seed, self._episode = int(seed), 0

    def next_episode_seed(self):
        s = (self._seed + self._episode) & 0xFFFFFFFF
        self._episode += 1
        return s

    @property
    def unwrapped(self):
        return self


MJMAZE_ENV_ID = 'HardMaze-v0'


class HardMazeEnv(PendulumEnv):
    """The spaces of the deceptive hard maze (csrc/maze.h under csrc/mjmaze.h) behind the same surface: a Box observation of shape (11,), a Box
    action of shape (2,) with bounds +-0.5 -- the values the maze clamps its two raw outputs to --, 400 steps.  There is no reset seed: every
    episode starts from the maze file's start point.  It holds the maze file as maze_run.maze_file resolves it (exp['maze_file'], hard_maze.txt
    in the working directory, the copy among the test fixtures)."""
    max_episode_steps = _lib.MJMAZE_STEPS

    def __init__(self, engine=None, seed=0, exp=None):
        from .maze_run import maze_file
        PendulumEnv.__init__(self, engine, seed)
        self.observation_space = _Space(shape=(_lib.MJMAZE_OBS,))
        self.action_space = _Space(shape=(_lib.MJMAZE_ADIM,))
        self.action_space.low = np.full(_lib.MJMAZE_ADIM, _lib.MJMAZE_AC_LOW, np.float32)
        self.action_space.high = np.full(_lib.MJMAZE_ADIM, _lib.MJMAZE_AC_HIGH, np.float32)
        self.maze_file = maze_file(exp or {})
        self.header, self.lines = _lib.load_maze(self.maze_file)


def mujoco_layout(hidden, n_out, n_obs=_lib.PENDULUM_OBS):
    """flat_layout for MujocoPolicy with two hidden layers of one width: TF's creation order, tf_util.dense's shapes (w [in][out], b [out])"""
    spec, o = OrderedDict(), 0
    for name, shape in (("l0/w", (n_obs, hidden)), ("l0/b", (hidden,)), ("l1/w", (hidden, hidden)), ("l1/b", (hidden,)),
                        ("out/w", (hidden, n_out)), ("out/b", (n_out,))):
        spec[name] = (o, shape)
        o += int(np.prod(shape))
    return spec, o


def mujoco_shape(ac_bins, nonlin_type, hidden_dims, connection_type, adim=1):
    """(hidden width, outputs, action mode, nonlinearity) of a MujocoPolicy csrc/pendulum.h (adim = 1 action dimension) or csrc/mjmaze.h (2)
    builds; everything else is refused by name.  The outputs are adim under the continuous action and adim * B under B uniform bins a
    dimension, at most 16 in all: B is bounded by 16 on the pendulum and by 8 on the maze."""
    if connection_type != 'ff':
        raise NotImplementedError("MujocoPolicy: connection_type {!r} (the reference itself builds only 'ff', policies.py:157-162)".format(connection_type))
    hidden_dims = list(hidden_dims)
    if len(hidden_dims) != 2:
        raise NotImplementedError("MujocoPolicy: hidden_dims {} -- the HIP engine builds exactly two hidden layers (every shipped configuration has [256, 256])".format(hidden_dims))
    if hidden_dims[0] != hidden_dims[1]:
        raise NotImplementedError("MujocoPolicy: hidden_dims {} -- the two hidden layers must have one width".format(hidden_dims))
    if hidden_dims[0] not in (64, 128, 256):
        raise NotImplementedError("MujocoPolicy: hidden width {} -- the HIP engine builds 64, 128 and 256".format(hidden_dims[0]))
    if nonlin_type not in _lib.PENDULUM_NONLINS:
        raise NotImplementedError("MujocoPolicy: nonlin_type {!r} -- the HIP engine builds 'tanh' and 'relu' ('lrelu' and 'elu' are not built)".format(nonlin_type))
    if not isinstance(ac_bins, str) or ':' not in ac_bins:
        raise NotImplementedError("MujocoPolicy: ac_bins {!r} -- 'continuous:' or 'uniform:B' expected".format(ac_bins))
    mode, arg = ac_bins.split(':')
    if mode == 'continuous':
        n_out = adim
    elif mode == 'uniform':
        n_out = int(arg) * adim
        if not 2 <= int(arg) <= _lib.PENDULUM_MAX_OUT // adim:
            raise NotImplementedError("MujocoPolicy: ac_bins {!r} -- the HIP engine builds 2..{} uniform bins".format(ac_bins, _lib.PENDULUM_MAX_OUT // adim))
    else:
        raise NotImplementedError("MujocoPolicy: ac_bins {!r} -- the HIP engine builds 'continuous:' and 'uniform:B' ('custom:' bins are not built)".format(ac_bins))
    return int(hidden_dims[0]), n_out, mode, nonlin_type


def refuse_mujoco(exp, driver):
    """nses / ga with MujocoPolicy.  The reference's novelty vector for this policy is the final (x_pos, y_pos) of MuJoCo's centre of mass
    (policies.py:252-256, 292-299).  The pendulum has no position, so there the two drivers are refused.  The hard maze has one -- the
    navigator's final (x, y) -- so nses lets 'HardMaze-v0' through (NS-ES and NSR-ES; nses.py's MujocoPolicy path); ga.py's own setup keeps
    refusing the policy: its Deep GA has drivers of its own (ga_mujoco.py), which the message names."""
    pointer = " -- its Deep GA is dne_hip.ga_mujoco (setup, run_master, run_worker), called directly" if driver == 'ga' else ""
    if exp['policy']['type'] == 'MujocoPolicy' and exp.get('env_id') == MJMAZE_ENV_ID:
        if driver == 'nses':
            return
        raise NotImplementedError("{} with MujocoPolicy is not built -- MujocoPolicy runs under es and nses (NS-ES, NSR-ES) on {} and under es "
                                  "on {}{}".format(driver, MJMAZE_ENV_ID, PENDULUM_ENV_ID, pointer))
    if exp['policy']['type'] == 'MujocoPolicy':
        raise NotImplementedError("{} with MujocoPolicy is not built: its behaviour characterisation is MuJoCo's centre of mass, and no simulator "
                                  "runs here -- MujocoPolicy runs under es on {}{}".format(driver, PENDULUM_ENV_ID, pointer))


def normc_flat(hidden, n_out, seed=0, n_obs=_lib.PENDULUM_OBS):
    """Initial MujocoPolicy parameters: U.normc_initializer(1.0) for the hidden layers and (0.01) for `out` -- randn columns scaled to that
    norm, tf_util.py:108-116 --, zero biases; drawn from RandomState(seed) in creation order (TF's own initialiser is unseeded)"""
    spec, P = mujoco_layout(hidden, n_out, n_obs)
    rs = np.random.RandomState(seed)
    th = np.zeros(P, np.float32)
    for name, (off, shape) in spec.items():
        if name.endswith('/w'):
            out = rs.randn(*shape).astype(np.float32)
            out *= (0.01 if name.startswith('out') else 1.0) / np.sqrt(np.square(out).sum(axis=0, keepdims=True))
            th[off:off + out.size] = out.reshape(-1)
    return th


class MujocoPolicy(Policy):
    """policies.py:122-217 with connection_type 'ff' and two hidden layers of one width, on the pendulum swing-up (the simulator the reference
    drives it on is not available): clip((ob - ob_mean) / ob_std, +-5) -> dense H, nonlin -> dense H, nonlin -> out, continuous or uniform bins;
    Gaussian action noise of ac_noise_std in training rollouts.  The network is csrc/pendulum.h: the engine's kernel for whole populations, the
    same text compiled for the CPU for act / rollout of the single current theta.  (The environment itself can be stepped on the device under
    any policy's actions: envs.make('Pendulum-v0', n), csrc/step_env.h.)"""
    kind = _lib.KIND_PENDULUM          # (an instance on the hard maze's spaces carries KIND_MJMAZE)

    def __init__(self, ob_space, ac_space, ac_bins, ac_noise_std, nonlin_type, hidden_dims, connection_type, engine=None):
        assert len(ob_space.shape) == len(ac_space.shape) == 1                                # policies.py:130
        # the layout comes from the observation width: 3 -> the pendulum (csrc/pendulum.h), 11 -> the hard maze (csrc/mjmaze.h)
        self.on_maze = (tuple(ob_space.shape), tuple(ac_space.shape)) == ((_lib.MJMAZE_OBS,), (_lib.MJMAZE_ADIM,))
        self.n_obs, adim = (_lib.MJMAZE_OBS, _lib.MJMAZE_ADIM) if self.on_maze else (_lib.PENDULUM_OBS, 1)
        self.hidden, self.n_out, self.ac_mode, self.nonlin = mujoco_shape(ac_bins, nonlin_type, hidden_dims, connection_type, adim)
        assert np.all(np.isfinite(ac_space.low)) and np.all(np.isfinite(ac_space.high)), 'Action bounds required'
        if not self.on_maze and (tuple(ob_space.shape) != (_lib.PENDULUM_OBS,) or tuple(ac_space.shape) != (1,)):
            raise NotImplementedError("MujocoPolicy: observation space {} and action space {} -- the HIP engine runs it on {} only, (3,) and (1,); "
                                      "no MuJoCo simulator is available".format(tuple(ob_space.shape), tuple(ac_space.shape), PENDULUM_ENV_ID))
        self.args = (ob_space, ac_space)
        self.kwargs = dict(ac_bins=ac_bins, ac_noise_std=ac_noise_std, nonlin_type=nonlin_type, hidden_dims=list(hidden_dims), connection_type=connection_type)
        self.ob_space_shape, self.ac_space, self.num_actions = tuple(ob_space.shape), ac_space, adim   # num_actions: the action's dimension (snapshots)
        self.ac_bins, self.ac_noise_std, self.hidden_dims, self.connection_type = ac_bins, float(ac_noise_std), list(hidden_dims), connection_type
        self.spec, self.num_params = mujoco_layout(self.hidden, self.n_out, self.n_obs)
        if self.on_maze:
            self.kind = _lib.KIND_MJMAZE
            assert self.num_params == _lib.mjmaze_num_params(self.hidden, self.n_out)
        else:
            assert self.num_params == _lib.pendulum_num_params(self.hidden, self.n_out)
        if engine is not None and (engine.kind != self.kind or engine.P != self.num_params or
                                   (getattr(engine, 'hidden', self.hidden), getattr(engine, 'n_actions', self.n_out)) != (self.hidden, self.n_out)):
            raise ValueError("MujocoPolicy: the engine passed in (kind {}, P {}) does not hold this policy ({} {}, P {})".format(
                engine.kind, engine.P, 'KIND_MJMAZE' if self.on_maze else 'KIND_PENDULUM', self.kind, self.num_params))
        self.engine = engine
        self._flat = np.zeros(self.num_params, np.float32)
        self.ob_mean = np.full(self.n_obs, np.nan, np.float32)                                 # policies.py:138-141
        self.ob_std = np.full(self.n_obs, np.nan, np.float32)

    @property
    def needs_ob_stat(self):
        return True

    @property
    def needs_ref_batch(self):
        return False

    def set_ob_stat(self, ob_mean, ob_std):
        self.ob_mean, self.ob_std = np.array(ob_mean, np.float32).reshape(-1), np.array(ob_std, np.float32).reshape(-1)
        if self.engine is not None:
            (self.engine.mjmaze_set_ob_stat if self.on_maze else self.engine.pendulum_set_ob_stat)(self.ob_mean, self.ob_std)

    def initialize(self, seed=0):
        self.set_trainable_flat(normc_flat(self.hidden, self.n_out, seed, self.n_obs))

    def reinitialize(self):
        """policies.py:42-44 over tf_util.py:149-158: every weight column of the current flat vector scaled to norm 1 -- std 1.0 for all three
        layers, `out` included: reinitialize never passes dense's own std --, every bias zero.  The arithmetic is csrc/mujoco_ga.h's host twin
        (the root of a genome, with the current vector as its noise slice)."""
        self.set_trainable_flat(_lib.mujoco_ga_theta_host(self.get_trainable_flat(), self.kind, self.hidden, self.n_out, (0, )))

    def set_from_seeds(self, seeds, noise_stdev, noise):
        """ga.py:152-158: the policy reinitialised on noise[seeds[0]], then v += noise_stdev * noise[seed] per further seed.  noise: the table
        the seeds index (a SharedNoiseTable or its array; ga.py reads its module's `noise`, a policy here holds none); the host twin computes
        it, bit for bit what the engine's bank holds for the same chain."""
        table = getattr(noise, 'noise', noise)
        seeds = [int(s) for s in seeds]
        genome = (seeds[0], ) + tuple((s, float(noise_stdev)) for s in seeds[1:])
        self.set_trainable_flat(_lib.mujoco_ga_theta_host(table, self.kind, self.hidden, self.n_out, genome))
        return self.get_trainable_flat()

    def _shape_kw(self):
        return dict(hidden=self.hidden, mean=self.ob_mean, std=self.ob_std, n_out=self.n_out, ac_mode=self.ac_mode, nonlin=self.nonlin)

    def act(self, ob, random_stream=None):
        """policies.py:202-206: actions [n][1] of observations [n][3] under the current theta (the hard maze: [n][2] of [n][11])"""
        ob = np.asarray(ob, np.float32).reshape(-1, self.n_obs)
        theta = np.broadcast_to(self.get_trainable_flat(), (ob.shape[0], self.num_params))
        forward = _lib.mjmaze_forward_host if self.on_maze else _lib.pendulum_forward_host
        a = forward(theta, ob, **self._shape_kw())[4].reshape(-1, self.num_actions)
        if random_stream is not None and self.ac_noise_std != 0:
            a = a + (random_stream.randn(*a.shape) * self.ac_noise_std).astype(np.float32)
        return a

    def rollout(self, env, *, render=False, timestep_limit=None, save_obs=False, random_stream=None, policy_seed=None):
        """policies.py:259-302: one episode of the current theta from env's next reset seed -> (rews float32 [T], T), with save_obs the
        observations acted on as well.  random_stream: the episode's 200 action-noise values are drawn from it (float32 of randn).  The
        reference's third value, MuJoCo's centre of mass, does not exist.
        On the hard maze (env: a HardMazeEnv): -> (rews, T, novelty_vector), novelty_vector float32 [2] = the final (x, y) -- the reference's
        final (x_pos, y_pos), policies.py:292-299; the episode's 800 action-noise values are drawn from random_stream."""
        if self.on_maze:
            return self._rollout_maze(env, timestep_limit, save_obs, random_stream, policy_seed)
        limit = _lib.PENDULUM_STEPS if timestep_limit is None else min(int(timestep_limit), _lib.PENDULUM_STEPS)
        if policy_seed:
            env.seed(policy_seed)
            if random_stream:
                random_stream.seed(policy_seed)
        noisy = random_stream is not None and self.ac_noise_std != 0
        table = random_stream.randn(_lib.PENDULUM_STEPS).astype(np.float32) if noisy else None
        r = _lib.pendulum_rollout_host(self.get_trainable_flat(), [env.next_episode_seed()], tslimit=limit, ac_noise_std=self.ac_noise_std,
                                       table=table, ac_off=[0] if noisy else None, want_trace=True, **self._shape_kw())
        tr = r['trace'][0, :limit]
        rews = tr[:, 5].astype(np.float32)
        if save_obs:
            return rews, limit, tr[:, :3].astype(np.float32)
        return rews, limit

    def _rollout_maze(self, env, timestep_limit, save_obs, random_stream, policy_seed):
        limit = _lib.MJMAZE_STEPS if timestep_limit is None else min(int(timestep_limit), _lib.MJMAZE_STEPS)
        if policy_seed and random_stream:
            random_stream.seed(policy_seed)
        noisy = random_stream is not None and self.ac_noise_std != 0
        table = random_stream.randn(_lib.MJMAZE_AC_NOISE).astype(np.float32) if noisy else None
        r = _lib.mjmaze_rollout_host(self.get_trainable_flat(), env.header, env.lines, tslimit=limit, ac_noise_std=self.ac_noise_std, table=table,
                                     ac_off=[0] if noisy else None, want_trace=save_obs, **self._shape_kw())
        rews = np.zeros(limit, np.float32)
        rews[-1] = r['returns'][0]                    # 0 until step 400, then minus the distance to the goal (a shorter episode: 0 throughout)
        nov = r['xy'][0].copy()
        if save_obs:
            return rews, limit, r['trace'][0, :limit, :_lib.MJMAZE_OBS].copy(), nov
        return rews, limit, nov

    def extra_variable_arrays(self, scope):
        """the two non-trainable variables of policies.py:138-141, after the trainable ones as all_variables lists them"""
        return OrderedDict([('%s/ob_mean:0' % scope, self.ob_mean.copy()), ('%s/ob_std:0' % scope, self.ob_std.copy())])

    def _spaces_blob(self):
        return _dumps_spaces(self.ob_space_shape, self.num_actions, self.kwargs, ac_box=(float(self.ac_space.low[0]), float(self.ac_space.high[0])))

    @classmethod
    def Load(cls, filename, engine=None, extra_kwargs=None):
        _, (ob_shape, adim), kwargs, arrays = cls._read_snapshot(filename)
        if extra_kwargs:
            kwargs.update(extra_kwargs)
        on_maze = (tuple(ob_shape), adim) == ((_lib.MJMAZE_OBS,), _lib.MJMAZE_ADIM)
        if not on_maze and (tuple(ob_shape) != (_lib.PENDULUM_OBS,) or adim != 1):
            raise NotImplementedError("MujocoPolicy.Load: a policy on observations {} and {} action dimensions -- the HIP engine runs it on {} "
                                      "only; no MuJoCo simulator is available".format(tuple(ob_shape), adim, PENDULUM_ENV_ID))
        env = HardMazeEnv() if on_maze else PendulumEnv()
        pol = cls(env.observation_space, env.action_space, engine=engine, **kwargs)
        pol._set_from_arrays(arrays, exact=True)
        pol.set_ob_stat(arrays['MujocoPolicy/ob_mean:0'], arrays['MujocoPolicy/ob_std:0'])
        return pol

    def initialize_from(self, filename, ob_stat=None):
        raise NotImplementedError("MujocoPolicy.initialize_from is not built (the snapshot the reference ships is 376 observations wide)")


class _GymBox(object):
    """stand-in whose pickle is renamed to gym.spaces.box.Box (state: low, high)"""


class _GymDiscrete(object):
    """stand-in whose pickle is renamed to gym.spaces.discrete.Discrete (state: n)"""


def _dumps_spaces(ob_shape, nact, kwargs, ac_box=None):
    """policies.py:56: `pickle.dumps((self.args, self.kwargs))` where args are the gym spaces the policy was built with.  A stock
    checkout's Policy.Load does `cls(*args, **kwargs)` and reads ob_space.shape / ac_space.n (policies.py:306-309, 434-438), so
    the pickle must name gym's classes -- whether or not gym is installed here, and without touching sys.modules (another thread
    may be importing or unpickling gym objects at this moment).  The two stand-in classes above are pickled under their own
    names and the GLOBAL opcodes are then renamed in the byte stream: protocol 2 writes a class reference as the text
    `c<module>\n<name>\n`, with no length field in front of it, so the replacement is exact.  The result is the pickle gym 0.9.4
    (requirements.txt:3) produces: Box state {low, high}, Discrete state {n}.
    The two bound arrays are written as `numpy.zeros(shape)` / `numpy.ones(shape)` calls rather than as 2 x 226 KB of buffer:
    smaller, and free of the numpy-version-specific module path (`numpy._core` vs `numpy.core`) of a pickled ndarray.
    ac_box = (low, high) scalars (MujocoPolicy): the action space is a Box of shape (nact,) with these bounds, written as `numpy.full` calls."""
    import io
    ob, ac = _GymBox(), (_GymDiscrete() if ac_box is None else _GymBox())
    ob.low, ob.high = np.zeros(ob_shape), np.ones(ob_shape)      # float64, as box.py builds them from scalar bounds
    if ac_box is None:
        ac.n = int(nact)
    else:
        ac.low, ac.high = np.full((int(nact),), float(ac_box[0])), np.full((int(nact),), float(ac_box[1]))

    class _Pickler(pickle.Pickler):
        def reducer_override(self, obj):
            if obj is ob.low:
                return np.zeros, (tuple(ob_shape),)
            if obj is ob.high:
                return np.ones, (tuple(ob_shape),)
            if ac_box is not None and obj is ac.low:
                return np.full, ((int(nact),), float(ac_box[0]))
            if ac_box is not None and obj is ac.high:
                return np.full, ((int(nact),), float(ac_box[1]))
            return NotImplemented
    out = io.BytesIO()
    _Pickler(out, protocol=2).dump(((ob, ac), kwargs))
    blob = out.getvalue()
    here = __name__.encode()
    for mine, (mod, name) in ((b'_GymBox', (b'gym.spaces.box', b'Box')), (b'_GymDiscrete', (b'gym.spaces.discrete', b'Discrete'))):
        if ac_box is not None and mine == b'_GymDiscrete':
            continue                 # (two Boxes: the class is written once, the second use is a memo reference)
        ref = b'c' + here + b'\n' + mine + b'\n'
        assert blob.count(ref) == 1, 'unexpected pickle layout'
        blob = blob.replace(ref, b'c' + mod + b'\n' + name + b'\n')
    return blob


def _loads_spaces(blob):
    """pickle.loads for a snapshot's 'args_and_kwargs' (policies.py:56: the policy's gym spaces + kwargs): where gym is not
    installed its space classes are stood in for by attribute bags, which is all Load needs (shape / n)."""
    import io

    class _Unpickler(pickle.Unpickler):
        def find_class(self, mod, name):
            try:
                return super().find_class(mod, name)
            except (ImportError, AttributeError):
                if mod.split('.')[0] != 'gym':
                    raise
                return type(name, (), {'__module__': mod})
    return _Unpickler(io.BytesIO(blob)).load()


def snapshot_extension():
    """'.h5' (es.py:288-291's snapshot_iter*.h5) when this machine can write HDF5 -- h5py, or libhdf5 through h5lite -- else '.npz'"""
    try:
        import h5py  # noqa: F401
        return '.h5'
    except ImportError:
        from . import h5lite
        return '.h5' if h5lite.available() else '.npz'
