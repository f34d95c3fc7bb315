"""What a gym.Acrobot-v1 driver (es_gpu, ga_gpu.dense_main / dense_ns_main, nses_gpu) does before its loop, as cartpole_run does for the
cart-pole: the game's and the models' names, the episode's step bound, and an engine with the noise table attached.  The acrobot has no engine
kind of its own: every run is a DNE_KIND_DENSE engine created on the environment id ENV_ACROBOT (csrc/acrobot.h, csrc/dense.h).  Imports none
of the drivers."""
from . import _lib
from .maze_run import MAZE_MODEL, attach_table

ACROBOT_GAME = 'gym.Acrobot-v1'          # gym_tensorflow.make sends every 'gym.*' name to GymEnv; this and 'gym.CartPole-v1' are the two built here
LINEAR_MODEL = 'LinearClassifier'        # neuroevolution/models/simple.py:23-27: 6 -> 3, P = 21
SIMPLE_MODEL = MAZE_MODEL                # SimpleClassifier (models/simple.py:29-35), here 6 -> 16 -> 16 -> 3 with relu, P = 435
MODEL_HIDDEN = {LINEAR_MODEL: (), SIMPLE_MODEL: (16, 16)}


def step_limit(tslimit):
    """the steps an episode may take: tslimit, at most Acrobot-v1's own 500 (GymEnv.reset ignores max_frames, tf_env.py:47-52), which None means"""
    return _lib.ACROBOT_STEPS if tslimit is None else min(int(tslimit), _lib.ACROBOT_STEPS)


def is_engine(engine):
    """a KIND_DENSE engine created on the acrobot"""
    return engine is not None and engine.kind == _lib.KIND_DENSE and getattr(engine, 'env_kind', None) == _lib.ENV_ACROBOT


def simple_name(engine, asked):
    """'SimpleClassifier' for an engine of that very shape when the run asks for the name; None: the shape's own name (es_gpu.dense_model_name)"""
    if asked == SIMPLE_MODEL and tuple(engine.hidden) == MODEL_HIDDEN[SIMPLE_MODEL] and engine.nonlin == _lib.DENSE_NONLINS['relu']:
        return SIMPLE_MODEL
    return None


def check_engine(engine):
    """a caller's engine has to be a KIND_DENSE one on the acrobot (None: open_engine makes one)"""
    if engine is not None and not is_engine(engine):
        raise ValueError("game {!r} asked for, the engine passed in (kind {} on environment kind {}) does not run it: a KIND_DENSE engine ({}) "
                         "created on ENV_ACROBOT ({}) does".format(ACROBOT_GAME, engine.kind, getattr(engine, 'env_kind', engine.kind),
                                                                   _lib.KIND_DENSE, _lib.ENV_ACROBOT))


def make_engine(max_members, model=LINEAR_MODEL):
    """a new KIND_DENSE engine on the acrobot of the shape `model` names: 'LinearClassifier' or 'SimpleClassifier'"""
    if model not in MODEL_HIDDEN:
        raise NotImplementedError("model {!r} on game {!r}: without an engine this loop runs {!r} and {!r} there".format(
            model, ACROBOT_GAME, LINEAR_MODEL, SIMPLE_MODEL))
    return _lib.Engine(_lib.KIND_DENSE, _lib.ACROBOT_ACTIONS, max_members=max_members, env=_lib.ENV_ACROBOT, hidden=MODEL_HIDDEN[model], nonlin='relu')


def open_engine(engine, noise, max_members, model=LINEAR_MODEL):
    """(engine, noise) of an acrobot run: the caller's or new ones (make_engine), the table attached"""
    check_engine(engine)
    if engine is None:
        engine = make_engine(max_members, model)
    return engine, attach_table(engine, noise)
