"""What every hard-maze driver (es_gpu, nses_gpu, ga_gpu) does the same way before its loop: the model's and the maze file's names, the
episode's step bound, and an engine of kind DNE_KIND_MAZE with the walls loaded and the noise table attached.  Imports none of the drivers."""
import os

from . import _lib
from .es import SharedNoiseTable

MAZE_MODEL = 'SimpleClassifier'          # the one model of exp['game'] == 'maze' (neuroevolution/models/simple.py:29-35)
MAZE_FILE = 'hard_maze.txt'              # tf_maze.py:28 names the file so, relative to the working directory; exp['maze_file'] overrides it
_MAZE_FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), 'tests', 'golden', 'hard_maze.txt')


def maze_file(exp):
    """the maze of a run: exp['maze_file'], else MAZE_FILE in the working directory, else the copy of the reference's file among the test fixtures"""
    path = exp.get('maze_file', MAZE_FILE)
    if os.path.exists(path):
        return path
    if 'maze_file' not in exp and os.path.exists(_MAZE_FIXTURE):
        return _MAZE_FIXTURE
    raise FileNotFoundError("maze file {!r} not found (exp['maze_file'] names it; the reference ships gym_tensorflow/maze/hard_maze.txt)".format(path))


def step_limit(tslimit):
    """the steps an episode may take: tslimit, at most env_default_timestep_cutoff (tf_maze.py:32-33), which None means"""
    return _lib.MAZE_STEPS if tslimit is None else min(int(tslimit), _lib.MAZE_STEPS)


def check_engine_kind(engine, game, kind, kind_name):
    """a caller's engine has to be of the kind that runs the game (None: the driver makes one); shared with cartpole_run"""
    if engine is not None and engine.kind != kind:
        raise ValueError("game {!r} asked for, the engine passed in is of kind {} ({} is {})".format(game, engine.kind, kind_name, kind))


def attach_table(engine, noise):
    """the run's noise table (the caller's, or a new SharedNoiseTable) attached to the engine; shared with cartpole_run"""
    noise = noise if noise is not None else SharedNoiseTable()
    noise.attach(engine)
    return noise


def check_engine(engine):
    """a caller's engine has to be of the maze's kind (None: open_engine makes one)"""
    check_engine_kind(engine, 'maze', _lib.KIND_MAZE, 'KIND_MAZE')


def open_engine(exp, engine, noise, max_members):
    """(engine, noise) of a maze run: the caller's or new ones, the walls of maze_file(exp) set, the table attached"""
    check_engine(engine)
    if engine is None:
        engine = _lib.Engine(_lib.KIND_MAZE, 2, max_members=max_members)
    engine.maze_set_walls(*_lib.load_maze(maze_file(exp)))
    return engine, attach_table(engine, noise)
