"""What an es or nses run of MujocoPolicy on the hard maze does before its loop, as pendulum_run does for Pendulum-v0: the environment id, the
episode's step bound, and an engine of kind DNE_KIND_MJMAZE in the policy's shape with the maze loaded.  Imports none of the drivers."""
from . import _lib
from .maze_run import check_engine_kind, maze_file
from .policies import MJMAZE_ENV_ID, mujoco_shape


def check_env_id(env_id):
    """exp['env_id'] of a MujocoPolicy experiment on the maze"""
    if env_id != MJMAZE_ENV_ID:
        raise NotImplementedError("MujocoPolicy on the hard maze: env_id {!r}; set \"env_id\": \"{}\"".format(env_id, MJMAZE_ENV_ID))


def step_limit(tslimit):
    """the steps an episode takes: tslimit, at most the maze's own 400, which None means"""
    return _lib.MJMAZE_STEPS if tslimit is None else min(int(tslimit), _lib.MJMAZE_STEPS)


def check_engine(engine):
    """a caller's engine has to be of the kind (None: open_engine makes one)"""
    check_engine_kind(engine, MJMAZE_ENV_ID, _lib.KIND_MJMAZE, 'KIND_MJMAZE')


def open_engine(exp, engine, max_members, device_id=0):
    """the engine of a MujocoPolicy experiment on the maze: the caller's, or a new one in the shape exp['policy']['args'] asks for (max_members
    0: only check the caller's); the walls of maze_file(exp) are set either way"""
    check_env_id(exp.get('env_id'))
    check_engine(engine)
    if engine is None:
        a = exp['policy']['args']
        hidden, n_out, ac_mode, nonlin = mujoco_shape(a['ac_bins'], a['nonlin_type'], a['hidden_dims'], a['connection_type'], _lib.MJMAZE_ADIM)
        engine = _lib.Engine(_lib.KIND_MJMAZE, n_out, max_members=max_members, device_id=device_id, hidden=hidden, ac_mode=ac_mode, nonlin=nonlin)
    engine.maze_set_walls(*_lib.load_maze(maze_file(exp)))
    return engine
