"""What an es run of MujocoPolicy does before its loop, as cartpole_run does for gym.CartPole-v1: the one environment id built here, the
episode's step bound, and an engine of kind DNE_KIND_PENDULUM in the policy's shape.  Imports none of the drivers."""
from . import _lib
from .maze_run import attach_table, check_engine_kind
from .policies import PENDULUM_ENV_ID, mujoco_shape

MUJOCO_IDS = ('Humanoid', 'HalfCheetah', 'Hopper', 'Walker2d', 'Ant', 'Swimmer', 'Reacher', 'InvertedPendulum', 'InvertedDoublePendulum')


def check_env_id(env_id):
    """exp['env_id'] of a MujocoPolicy experiment: Pendulum-v0, the one environment built here"""
    if env_id == PENDULUM_ENV_ID:
        return
    why = " (a MuJoCo environment: no simulator is available, the policy runs on {} instead)".format(PENDULUM_ENV_ID) \
        if str(env_id).split('-')[0] in MUJOCO_IDS else ""
    raise NotImplementedError("MujocoPolicy: env_id {!r} is not built{}; set \"env_id\": \"{}\"".format(env_id, why, PENDULUM_ENV_ID))


def step_limit(tslimit):
    """the steps an episode takes: tslimit, at most Pendulum-v0's own 200, which None means"""
    return _lib.PENDULUM_STEPS if tslimit is None else min(int(tslimit), _lib.PENDULUM_STEPS)


def check_engine(engine):
    """a caller's engine has to be of the pendulum's kind (None: open_engine makes one)"""
    check_engine_kind(engine, PENDULUM_ENV_ID, _lib.KIND_PENDULUM, 'KIND_PENDULUM')


def open_engine(exp, engine, max_members, device_id=0):
    """the engine of a MujocoPolicy experiment: the caller's, or a new one in the shape exp['policy']['args'] asks for"""
    check_env_id(exp.get('env_id'))
    check_engine(engine)
    if engine is None:
        a = exp['policy']['args']
        hidden, n_out, ac_mode, nonlin = mujoco_shape(a['ac_bins'], a['nonlin_type'], a['hidden_dims'], a['connection_type'])
        engine = _lib.Engine(_lib.KIND_PENDULUM, n_out, max_members=max_members, device_id=device_id, hidden=hidden, ac_mode=ac_mode, nonlin=nonlin)
    return engine
