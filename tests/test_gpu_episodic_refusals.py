"""GPU: what the four whole-episode kinds (DNE_KIND_MAZE, DNE_KIND_CARTPOLE, DNE_KIND_PENDULUM, DNE_KIND_MJMAZE) refuse, with the WHOLE text of
every refusal and, where more than one thing is wrong, the one that wins.  Each evaluation checks in its own order -- the maze: walls, limit,
bc, noise; the cart-pole: bc, limit, seed, noise; the pendulum: bc, limit, seed, noise, statistics, options; mjmaze: bc, limit, walls, noise,
statistics, options -- and the host glue of the four is shared, so a text or an order that moves shows here.  Every refusal is returned by
host code before any launch.  Engines of 4 members, hidden width 64, a four-wall maze, no evaluation longer than 8 steps.

(A member set needs a noise table -- dne_set_members checks every member's slice against it -- and a table is never taken away again, so the
evaluations' own "noise table not uploaded" cannot be reached through the C ABI; a fresh engine is refused earlier, and those texts are here.)"""
import ctypes as C

import numpy as np
import pytest

import maze_support as MS

pytestmark = pytest.mark.gpu
T = 8
BIG, SMALL = 8192, 6000          # two noise tables: every H = 64 theta (5058 floats at most) fits the small one, the big one's last offsets do not
NO_NOISE = "noise table not uploaded (dne_noise_upload)"
NO_LIMIT = "timestep limit must be positive"
NO_MAZE = "DNE_KIND_%s: no maze loaded (dne_maze_set_walls comes before an evaluation)"


def noise(n=BIG):
    return np.random.RandomState(3).randn(BIG).astype(np.float32)[:n]


def make(kind_name, **kw):
    from dne_hip import _lib
    kind = getattr(_lib, "KIND_" + kind_name)
    if kind in _lib.MUJOCO_KINDS:
        kw = dict(dict(hidden=64, ac_mode="continuous", nonlin="tanh"), **kw)
    return _lib.Engine(kind, 1 if kind == _lib.KIND_PENDULUM else 2, max_members=4, **kw)


def members(e, n):
    e.set_members(np.zeros(n, np.int32), np.arange(n, dtype=np.int64) * 7, np.full(n, 0.02, np.float32))


def refusal(fn):
    from dne_hip import _lib
    with pytest.raises(_lib.DneError) as ei:
        fn()
    return str(ei.value)


def raw_eval(e, call, n, tslimit, seeds=True, bc=False):
    """dne_eval_members / dne_es_eval (n members: n / 2 pairs) as the C ABI takes them, env_seed and bc NULL or not -> the refusal's text"""
    ret = np.zeros(n, np.float32); sg = np.zeros(n, np.float32); ln = np.zeros(n, np.int32)
    sd = np.zeros(n, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32)) if seeds else None
    bcbuf = np.zeros(n * 1024, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)) if bc else None
    out = [a.ctypes.data_as(C.POINTER(t)) for a, t in ((ret, C.c_float), (sg, C.c_float), (ln, C.c_int32))]
    if call == "dne_es_eval":
        idx = np.arange(n // 2, dtype=np.int64)
        rc = e.lib.dne_es_eval(e.h, idx.ctypes.data_as(C.POINTER(C.c_int64)), n // 2, C.c_float(0.02), int(tslimit), sd, *out, bcbuf)
    else:
        rc = e.lib.dne_eval_members(e.h, int(n), int(tslimit), sd, *out, bcbuf)
    assert rc != 0, "%s was not refused" % call
    return e.lib.dne_last_error(e.h).decode()


def raw(e, name, *args):
    assert getattr(e.lib, name)(e.h, *args) != 0, "%s was not refused" % name
    return e.lib.dne_last_error(e.h).decode()


SEEDS2 = np.zeros(2, np.uint32)


def test_maze():
    e = make("MAZE")
    try:
        # neither walls nor a noise table nor members: what each entry point says first
        assert refusal(lambda: e.eval_members(2, T, SEEDS2)) == "dne_eval_members: 2 members asked for, dne_set_members set 0"
        assert refusal(lambda: e.es_eval([0], 0.02, T, SEEDS2)) == NO_NOISE
        assert refusal(lambda: e.maze_debug_trace(0, T)) == NO_MAZE % "MAZE"
        assert refusal(lambda: e.maze_final_state(1)) == "dne_maze_final_state: 1 members asked for, the last evaluation ran 0"
        assert refusal(lambda: e.eval_members(5, T, np.zeros(5, np.uint32))) == "n = 5 outside [1, max_members = 4]"
        e.noise_upload(noise())
        members(e, 2)
        # no walls wins over a bad limit and over bc on an engine without record_bc
        assert raw_eval(e, "dne_eval_members", 2, 0, bc=True) == NO_MAZE % "MAZE"
        assert raw_eval(e, "dne_es_eval", 2, 0, bc=True) == NO_MAZE % "MAZE"
        header, lines = MS.synthetic_maze(4)
        assert refusal(lambda: e.maze_set_walls(header, lines[:0])) == "maze: 0 walls, the kernel and the host function take 1..64"
        assert refusal(lambda: e.maze_set_walls(header, np.zeros((65, 4), np.float32))) == "maze: 65 walls, the kernel and the host function take 1..64"
        assert raw(e, "dne_maze_set_walls", None, None, 4) == "maze: header or lines missing"
        e.maze_set_walls(header, lines)
        assert raw_eval(e, "dne_eval_members", 2, 0, bc=True) == NO_LIMIT
        assert raw_eval(e, "dne_eval_members", 2, T, bc=True) == "behaviour characterisations requested but the engine was created with record_bc = 0"
        assert raw_eval(e, "dne_eval_members", 3, T) == "dne_eval_members: 3 members asked for, dne_set_members set 2"
        assert refusal(lambda: e.maze_debug_trace(2, T)) == "dne_maze_debug_trace: member 2, dne_set_members set 2"
        assert refusal(lambda: e.maze_debug_trace(-1, T)) == "dne_maze_debug_trace: member -1, dne_set_members set 2"
        assert refusal(lambda: e.maze_debug_trace(0, 0)) == "dne_maze_debug_trace: bad arguments"
        assert raw(e, "dne_maze_debug_trace", 0, T, None) == "dne_maze_debug_trace: bad arguments"
        # a refused evaluation leaves the count of the last one alone; a finished one sets it
        assert refusal(lambda: e.maze_final_state(1)) == "dne_maze_final_state: 1 members asked for, the last evaluation ran 0"
        _, _, ln = e.eval_members(2, T, SEEDS2)
        assert ln.tolist() == [T, T] and e.maze_final_state(2).shape == (2, 2) and e.maze_debug_trace(1, T).shape == (T, 16)
        assert refusal(lambda: e.maze_final_state(3)) == "dne_maze_final_state: 3 members asked for, the last evaluation ran 2"
        assert refusal(lambda: e.maze_final_state(0)) == "dne_maze_final_state: 0 members asked for, the last evaluation ran 2"
        for call, name in ((lambda: e.cartpole_final_state(1), "dne_cartpole_final_state needs a DNE_KIND_CARTPOLE"),
                           (lambda: e.cartpole_debug_trace(0, T), "dne_cartpole_debug_trace needs a DNE_KIND_CARTPOLE"),
                           (lambda: e.pendulum_ob_stats(1), "dne_pendulum_ob_stats needs a DNE_KIND_PENDULUM"),
                           (lambda: e.pendulum_set_rollout_options(2), "dne_pendulum_set_rollout_options needs a DNE_KIND_PENDULUM"),
                           (lambda: e.pendulum_debug_trace(0, T), "dne_pendulum_debug_trace needs a DNE_KIND_PENDULUM"),
                           (lambda: e.mjmaze_set_ob_stat(np.zeros(11), np.ones(11)), "dne_mjmaze_set_ob_stat needs a DNE_KIND_MJMAZE"),
                           (lambda: e.mjmaze_set_rollout_options(2), "dne_mjmaze_set_rollout_options needs a DNE_KIND_MJMAZE"),
                           (lambda: e.mjmaze_ob_stats(1), "dne_mjmaze_ob_stats needs a DNE_KIND_MJMAZE"),
                           (lambda: e.mjmaze_debug_trace(0, T), "dne_mjmaze_debug_trace needs a DNE_KIND_MJMAZE")):
            assert refusal(call) == name + " engine (this one: kind 4)"
        e.check_redzones()
    finally:
        e.close()


def test_cartpole():
    e = make("CARTPOLE")
    try:
        assert refusal(lambda: e.eval_members(2, T, SEEDS2)) == "dne_eval_members: 2 members asked for, dne_set_members set 0"
        assert refusal(lambda: e.es_eval([0], 0.02, T, SEEDS2)) == NO_NOISE
        assert refusal(lambda: e.cartpole_debug_trace(0, T)) == "dne_cartpole_debug_trace: member 0, dne_set_members set 0"
        e.noise_upload(noise())
        members(e, 2)
        bc = ("%s: behaviour characterisations are not available on a DNE_KIND_CARTPOLE engine (kind 5): bc must be NULL; "
              "dne_cartpole_final_state has the final state of every member")
        seed = "%s: a DNE_KIND_CARTPOLE engine resets every member from its environment seed, env_seed is NULL"
        for call in ("dne_eval_members", "dne_es_eval"):
            assert raw_eval(e, call, 2, 0, seeds=False, bc=True) == bc % call        # bc wins over the limit and over a NULL env_seed
            assert raw_eval(e, call, 2, T, seeds=False, bc=True) == bc % call
            assert raw_eval(e, call, 2, 0, seeds=False) == NO_LIMIT                  # the limit wins over a NULL env_seed
            assert raw_eval(e, call, 2, T, seeds=False) == seed % call
        assert refusal(lambda: e.cartpole_final_state(1)) == "dne_cartpole_final_state: 1 members asked for, the last evaluation ran 0"
        assert refusal(lambda: e.cartpole_debug_trace(2, T)) == "dne_cartpole_debug_trace: member 2, dne_set_members set 2"
        assert refusal(lambda: e.cartpole_debug_trace(0, 0)) == "dne_cartpole_debug_trace: bad arguments"
        steps = C.c_int32(0)
        assert raw(e, "dne_cartpole_debug_trace", 0, T, None, None, C.byref(steps)) == "dne_cartpole_debug_trace: bad arguments"
        _, _, ln = e.eval_members(2, T, SEEDS2)
        assert ln.max() <= T and e.cartpole_final_state(2).shape == (2, 4) and e.cartpole_debug_trace(0, T).shape == (ln[0], 8)
        assert refusal(lambda: e.cartpole_final_state(3)) == "dne_cartpole_final_state: 3 members asked for, the last evaluation ran 2"
        assert raw(e, "dne_cartpole_final_state", 1, None) == "dne_cartpole_final_state: no output buffer"
        for call, name in ((lambda: e.maze_final_state(1), "dne_maze_final_state needs a DNE_KIND_MAZE"),
                           (lambda: e.maze_set_walls(*MS.synthetic_maze(4)), "dne_maze_set_walls needs a DNE_KIND_MAZE"),
                           (lambda: e.pendulum_final_state(1), "dne_pendulum_final_state needs a DNE_KIND_PENDULUM"),
                           (lambda: e.mjmaze_ob_stats(1), "dne_mjmaze_ob_stats needs a DNE_KIND_MJMAZE")):
            assert refusal(call) == name + " engine (this one: kind 5)"
        e.check_redzones()
    finally:
        e.close()


def _mujoco(kind_name, prefix, obs_w, ac_values, kind, final_state):
    """the refusals DNE_KIND_PENDULUM and DNE_KIND_MJMAZE share, text by text; ac_values: the action-noise values a member reads"""
    KIND = "DNE_KIND_" + kind_name
    is_maze = kind_name == "MJMAZE"
    e = make(kind_name)
    set_stat = getattr(e, prefix + "_set_ob_stat")
    set_opt = getattr(e, prefix + "_set_rollout_options")
    ob_stats = getattr(e, prefix + "_ob_stats")
    trace = getattr(e, prefix + "_debug_trace")
    nan_stat = "%s: the observation statistics of a " + KIND + " engine are NaN until dne_" + prefix + "_set_ob_stat is called"
    try:
        assert refusal(lambda: e.eval_members(2, T, SEEDS2)) == "dne_eval_members: 2 members asked for, dne_set_members set 0"
        assert refusal(lambda: e.es_eval([0], 0.02, T, SEEDS2)) == NO_NOISE
        assert refusal(lambda: trace(0, T)) == "dne_%s_debug_trace: member 0, dne_set_members set 0" % prefix
        assert refusal(lambda: set_opt(2, 0.01, np.zeros(2, np.int64))) == NO_NOISE
        assert refusal(lambda: set_opt(5, 0.01)) == "n = 5 outside [1, max_members = 4]"
        assert raw(e, "dne_%s_set_ob_stat" % prefix, None, None) == "dne_%s_set_ob_stat: bad arguments" % prefix
        e.noise_upload(noise())
        members(e, 2)
        bc = "%s: behaviour characterisations are not available on a " + KIND + " engine (kind %d): bc must be NULL; " % kind + final_state
        for call in ("dne_eval_members", "dne_es_eval"):
            assert raw_eval(e, call, 2, 0, seeds=False, bc=True) == bc % call      # bc wins over everything else that is wrong
            assert raw_eval(e, call, 2, 0, seeds=False) == NO_LIMIT                # then the limit
            if is_maze:                                                            # then the walls (env_seed is not read), then the statistics
                assert raw_eval(e, call, 2, T, seeds=False) == NO_MAZE % "MJMAZE"
            else:                                                                  # then the seed, then the statistics
                assert raw_eval(e, call, 2, T, seeds=False) == "%s: a DNE_KIND_PENDULUM engine resets every member from its environment seed, env_seed is NULL" % call
        if is_maze:
            assert refusal(lambda: trace(0, T)) == NO_MAZE % "MJMAZE"
            e.maze_set_walls(*MS.synthetic_maze(4))
        # options for 4 members with an offset that a smaller table will not hold; the statistics are still missing
        last = BIG - ac_values
        past = "dne_%s_set_rollout_options: member 1 reads its %d action-noise values from offset %d, past the noise table's %d values"
        assert refusal(lambda: set_opt(2, 0.01, np.array([0, last + 1], np.int64))) == past % (prefix, ac_values, last + 1, BIG)
        set_opt(4, 0.01, np.array([-1, last, 0, -1], np.int64), np.array([1, 0, 1, 0], np.uint8))
        e.noise_upload(noise(SMALL))
        members(e, 2)
        assert raw_eval(e, "dne_eval_members", 2, T) == nan_stat % "dne_eval_members"          # the statistics win over the options
        assert raw_eval(e, "dne_es_eval", 2, T) == nan_stat % "dne_es_eval"
        assert refusal(lambda: trace(0, T)) == nan_stat % ("dne_%s_debug_trace" % prefix)
        set_stat(np.zeros(obs_w, np.float32), np.ones(obs_w, np.float32))
        # options given for another n win over the offset past the table; a refused evaluation keeps the options
        given = "%s: dne_" + prefix + "_set_rollout_options was given 4 members, this evaluation runs 2"
        assert raw_eval(e, "dne_eval_members", 2, T) == given % "dne_eval_members"
        assert raw_eval(e, "dne_es_eval", 2, T) == given % "dne_es_eval"
        members(e, 4)
        off = "%s: member 1 reads its action noise from offset %d, past the noise table's %d values"
        assert raw_eval(e, "dne_eval_members", 4, T) == off % ("dne_eval_members", last, SMALL)
        assert raw_eval(e, "dne_es_eval", 4, T) == off % ("dne_es_eval", last, SMALL)
        assert refusal(lambda: ob_stats(1)) == "dne_%s_ob_stats: 1 members asked for, the last evaluation ran 0" % prefix
        # the trace ignores the options and leaves them; an evaluation that runs clears them
        assert trace(0, T).shape[0] <= T
        assert raw_eval(e, "dne_eval_members", 4, T) == off % ("dne_eval_members", last, SMALL)
        set_opt(4, 0.01, np.array([-1, SMALL - ac_values, 0, -1], np.int64), np.array([1, 0, 1, 0], np.uint8))
        _, _, ln = e.eval_members(4, T, np.arange(4, dtype=np.uint32))
        s, q, c = ob_stats(4)
        assert ln.max() <= T and c.tolist() == [ln[0], 0, ln[2], 0] and s.shape == q.shape == (4, obs_w)
        members(e, 2)
        _, _, ln = e.eval_members(2, T, SEEDS2)                                     # (no "was given 4 members": the options are gone)
        assert ob_stats(2)[2].tolist() == [0, 0]
        assert refusal(lambda: ob_stats(3)) == "dne_%s_ob_stats: 3 members asked for, the last evaluation ran 2" % prefix
        n = np.zeros(4, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        assert raw(e, "dne_%s_ob_stats" % prefix, 1, n, n, None) == "dne_%s_ob_stats: no output buffer" % prefix
        assert refusal(lambda: trace(2, T)) == "dne_%s_debug_trace: member 2, dne_set_members set 2" % prefix
        assert refusal(lambda: trace(0, 0)) == "dne_%s_debug_trace: bad arguments" % prefix
        e.check_redzones()
        return e
    except BaseException:
        e.close()
        raise


def test_pendulum():
    e = _mujoco("PENDULUM", "pendulum", 3, 200, 6, "dne_pendulum_final_state has the final state of every member")
    try:
        assert e.pendulum_final_state(2).shape == (2, 2)
        assert refusal(lambda: e.pendulum_final_state(3)) == "dne_pendulum_final_state: 3 members asked for, the last evaluation ran 2"
        assert raw(e, "dne_pendulum_final_state", 1, None) == "dne_pendulum_final_state: no output buffer"
        for call, name in ((lambda: e.maze_final_state(1), "dne_maze_final_state needs a DNE_KIND_MAZE"),
                           (lambda: e.cartpole_debug_trace(0, T), "dne_cartpole_debug_trace needs a DNE_KIND_CARTPOLE"),
                           (lambda: e.mjmaze_set_ob_stat(np.zeros(11), np.ones(11)), "dne_mjmaze_set_ob_stat needs a DNE_KIND_MJMAZE"),
                           (lambda: e.mjmaze_debug_trace(0, T), "dne_mjmaze_debug_trace needs a DNE_KIND_MJMAZE")):
            assert refusal(call) == name + " engine (this one: kind 6)"
    finally:
        e.close()


def test_mjmaze():
    e = _mujoco("MJMAZE", "mjmaze", 11, 800, 7, "dne_maze_final_state has the final (x, y) of every member")
    try:
        assert e.maze_final_state(2).shape == (2, 2)                                # mjmaze sets the maze's count with its own
        assert refusal(lambda: e.maze_final_state(3)) == "dne_maze_final_state: 3 members asked for, the last evaluation ran 2"
        for call, name in ((lambda: e.maze_debug_trace(0, T), "dne_maze_debug_trace needs a DNE_KIND_MAZE"),
                           (lambda: e.cartpole_final_state(1), "dne_cartpole_final_state needs a DNE_KIND_CARTPOLE"),
                           (lambda: e.pendulum_ob_stats(1), "dne_pendulum_ob_stats needs a DNE_KIND_PENDULUM"),
                           (lambda: e.pendulum_final_state(1), "dne_pendulum_final_state needs a DNE_KIND_PENDULUM")):
            assert refusal(call) == name + " engine (this one: kind 7)"
    finally:
        e.close()
