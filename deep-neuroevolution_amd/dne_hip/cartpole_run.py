"""What a gym.CartPole-v1 driver (es_gpu) does before its loop, as maze_run does for the hard maze: the game's and the model's names, the
episode's step bound, and an engine of kind DNE_KIND_CARTPOLE with the noise table attached.  Imports none of the drivers."""
from . import _lib
from .maze_run import MAZE_MODEL, attach_table, check_engine_kind

CARTPOLE_GAME = 'gym.CartPole-v1'        # configurations/es_gym_config.json; gym_tensorflow.make sends every 'gym.*' name to GymEnv, this is the one built here
CARTPOLE_MODEL = MAZE_MODEL              # SimpleClassifier (neuroevolution/models/simple.py:29-35), here on 4 inputs


def step_limit(tslimit):
    """the steps an episode may take: tslimit, at most CartPole-v1's own 500 (GymEnv.reset ignores max_frames, tf_env.py:47-52), which None means"""
    return _lib.CARTPOLE_STEPS if tslimit is None else min(int(tslimit), _lib.CARTPOLE_STEPS)


def check_engine(engine):
    """a caller's engine has to be of the cart-pole's kind (None: open_engine makes one)"""
    check_engine_kind(engine, CARTPOLE_GAME, _lib.KIND_CARTPOLE, 'KIND_CARTPOLE')


def open_engine(engine, noise, max_members):
    """(engine, noise) of a cart-pole run: the caller's or new ones, the table attached"""
    check_engine(engine)
    if engine is None:
        engine = _lib.Engine(_lib.KIND_CARTPOLE, 2, max_members=max_members)
    return engine, attach_table(engine, noise)
