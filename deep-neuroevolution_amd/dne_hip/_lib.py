"""ctypes shim over libdne_hip.so (include/dne_hip.h) -- the only way Python reaches the HIP kernels.

There is no CPU fallback: if the shared library is missing, or no MI355X is visible, constructing an
Engine raises.  numpy arrays cross the boundary as plain pointers + sizes.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
LIB_PATH = os.environ.get("DNE_LIB_PATH") or os.path.join(_CSRC, "libdne_hip.so")   # DNE_LIB_PATH: another build of the same ABI (same-box A/B of whole builds)

KIND_ES, KIND_GA, KIND_GA_LARGE = 0, 1, 2   # DNE_KIND_* (include/dne_hip.h); 2 = the GPU tree's LargeModel (models/dqn.py:39-47)
KIND_ES_VBN = 3   # the GPU tree's ModelVirtualBN in its own flat layout (models/batchnorm.py:52-123): the ES kind's network and entry points
KIND_MAZE = 4     # the GPU tree's hard maze under SimpleClassifier (gym_tensorflow/maze/, models/simple.py:29-35): whole episodes in one kernel (csrc/maze.h)
MAZE_OBS, MAZE_STEPS, MAZE_TRACE_W, MAZE_MAX_WALLS = 11, 400, 16, 64   # observation width, tf_maze.cpp's episode length, floats per trace row, walls the kernel takes
RAM_NOVELTY_KMAX, RAM_NOVELTY_TILE, RAM_NOVELTY_MEMBERS = 32, 256, 4   # DNE_RAM_NOVELTY_* (csrc/ram_novelty.h): neighbours a lane keeps, combined slots per LDS tile, members per workgroup
DENSE_NOVELTY_KMAX = 32   # DNE_DENSE_NOVELTY_KMAX = DNE_MAZE_NOVELTY_KMAX (csrc/dense_novelty.h uses maze_novelty.h's list)
MAZE_NOVELTY_KMAX, MAZE_NOVELTY_TILE, MAZE_ARCHIVE_CAP0 = 32, 1024, 64   # csrc/maze_novelty.h: neighbours a lane keeps, archive points per LDS tile; the archive's first allocation (engine.hip)
KIND_CARTPOLE = 5   # the GPU tree's gym configuration: gym.CartPole-v1 under SimpleClassifier on 4 inputs, whole episodes in one kernel (csrc/cartpole.h)
CARTPOLE_OBS, CARTPOLE_STEPS, CARTPOLE_TRACE_W, CARTPOLE_P = 4, 500, 8, 386   # observation width, CartPole-v1's max_episode_steps, doubles per trace row, parameters
KIND_PENDULUM = 6   # es_distributed's MujocoPolicy on the torque-limited pendulum swing-up, whole episodes in one kernel (csrc/pendulum.h)
PENDULUM_OBS, PENDULUM_STEPS, PENDULUM_TRACE_W, PENDULUM_MAX_OUT = 3, 200, 8, 16   # observation width, Pendulum-v0's max_episode_steps, doubles per trace row, most bins
PENDULUM_AC_MODES = {'continuous': 0, 'uniform': 1}   # dne_config.reserved[1]
PENDULUM_NONLINS = {'tanh': 0, 'relu': 1}             # dne_config.reserved[2]
PENDULUM_MATH = {'tanh': 0, 'norm': 1, 'normalise': 2}   # dne_pendulum_debug_math / _math_host
KIND_MJMAZE = 7   # MujocoPolicy on the hard maze (final (x, y) as the behaviour characterisation), whole episodes in one kernel (csrc/mjmaze.h)
MJMAZE_OBS, MJMAZE_ADIM, MJMAZE_STEPS, MJMAZE_TRACE_W, MJMAZE_MAX_BINS = 11, 2, 400, 20, 8   # observations, action dimensions, steps, floats per trace row, most bins a dimension
MJMAZE_AC_NOISE = MJMAZE_ADIM * MJMAZE_STEPS            # action-noise values an episode reads from the table
MJMAZE_AC_LOW, MJMAZE_AC_HIGH = -0.5, 0.5               # the action space: what the maze clamps its raw outputs to
KIND_DENSE = 8    # a dense policy of any small shape (0..3 hidden layers of width 1..64) on the maze, the cart-pole, the pendulum or the acrobot (csrc/dense.h)
ENV_ACROBOT = 9   # DNE_ENV_ACROBOT: gym.Acrobot-v1 (csrc/acrobot.h), an environment id -- no engine kind: a KIND_DENSE engine is created on it (env=ENV_ACROBOT, 3 outputs)
ACROBOT_OBS, ACROBOT_STEPS, ACROBOT_ACTIONS = 6, 500, 3   # observation width, Acrobot-v1's max_episode_steps, actions (torque -1 / 0 / +1)
DENSE_NONLINS = {'tanh': 0, 'relu': 1}                # dne_config.reserved[2] of a KIND_DENSE engine
MUJOCO_KINDS = (KIND_PENDULUM, KIND_MJMAZE)             # the kinds whose shape travels in dne_config.reserved
ES_KINDS = (KIND_ES, KIND_ES_VBN)   # virtual batch norm over a reference batch, antithetic pairs
PROC_MODES = {"centered_rank": 0, "sign": 1, "centered_sign_rank": 2}
OPT_KINDS = {"adam": 0, "sgd": 1}
OB_SHAPE = (84, 84, 4)
OB_BYTES = 84 * 84 * 4
RAM_BYTES = 128
BN_FLOATS = 608
# gym registers *NoFrameskip-v4 with max_episode_steps = 400000, counted by its TimeLimit wrapper in steps of the RAW environment
# (frames).  policies.py:383-385 reads that number through env.spec and applies it as a bound on AGENT steps (one per 4 frames),
# while the real TimeLimit sits inside the wrappers and would end the episode after 100000 agent steps.  The mirror keeps the
# reference's arithmetic as written (min(task limit, 400000) agent steps): 4x looser than gym's own limit, never reached by the
# BASELINE configurations (tslimit 5000) -- DESIGN.md section 5.
ENV_MAX_EPISODE_STEPS = 400000


class DneError(RuntimeError):
    pass


# one (noise_idx, returns, lengths, sign-returns) record per antithetic pair -- what travels between GPUs;
# the layout of struct PairRecord in csrc/reduce.h
RECORD = np.dtype([('noise_idx', '<i8'), ('ret', '<f4', (2,)), ('len', '<i4', (2,)), ('aux', '<f4', (2,))])
assert RECORD.itemsize == 32


def comm_unique_id():
    """ncclGetUniqueId through the C ABI (rank 0 calls it and hands the 128 bytes to every rank)"""
    buf = (C.c_char * 128)()
    if load().dne_comm_unique_id(buf) != 0:
        raise DneError(load().dne_last_error(None).decode())
    return bytes(buf.raw)


def device_count():
    """HIP devices visible to this process (0 without a GPU)"""
    n = C.c_int(0)
    if load().dne_device_count(C.byref(n)) != 0:
        raise DneError(load().dne_last_error(None).decode())
    return n.value


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("device_id", "policy_kind", "n_actions", "max_members", "ref_count",
                                         "ref_chunk", "record_bc", "bc_max_steps", "profile_events", "bc_final_only")] + \
               [("reserved", C.c_int32 * 6)]


class Profile(C.Structure):
    _fields_ = [("eval_ms", C.c_double), ("fc_ms", C.c_double), ("fc_launches", C.c_int64),
                ("fc_group_steps", C.c_int64), ("env_steps", C.c_int64), ("conv_ms", C.c_double),
                ("env_ms", C.c_double), ("ref_ms", C.c_double), ("reduce_ms", C.c_double),
                ("materialize_ms", C.c_double), ("fc_full_ms", C.c_double), ("fc_full_launches", C.c_double),
                ("fc_full_units", C.c_double), ("fc_full_kind", C.c_double), ("fc_full_union_ms", C.c_double), ("reserved", C.c_double * 1)]


def build(force=False):
    """Compile libdne_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in ("engine.hip", "plan.h", "forward.h", "forward_variants.h", "forward_large.h", "reduce.h", "novelty.h", "env_synth.h", "maze.h", "maze_novelty.h", "maze_ga.h", "cartpole.h", "pendulum.h", "mjmaze.h", "step_env.h", "dense.h", "dense_ga.h", "mujoco_ga.h", "dense_novelty.h", "ram_novelty.h")]
    srcs.append(os.path.join(os.path.dirname(os.path.dirname(_CSRC)), "include", "dne_hip.h"))
    if os.environ.get("DNE_LIB_PATH"):
        # another build of the same ABI was asked for by name: `make` only knows the in-tree library, so running it here would
        # rebuild THAT one in the middle of an A/B and still not produce the file named -- check the file and leave it alone
        if not os.path.exists(LIB_PATH):
            raise DneError("DNE_LIB_PATH=%s does not exist (it names a prebuilt library; nothing is built for it)" % LIB_PATH)
        return LIB_PATH
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        subprocess.check_call(["make", "-C", _CSRC, "-s"])
    return LIB_PATH


_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DneError("libdne_hip.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "-- the HIP engine has no CPU fallback" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.dne_last_error.restype = C.c_char_p
        lib.dne_last_error.argtypes = [C.c_void_p]
        lib.dne_destroy.restype = None
        _mujoco_ga_argtypes(lib)
        _lib = lib
    return _lib


def _mujoco_ga_argtypes(lib):
    """dne_mujoco_ga_* (include/dne_hip.h): every argument typed, so that a wrong one is a ctypes.ArgumentError and not a wild pointer"""
    P = C.POINTER
    h, i32, i64, f32, u32 = C.c_void_p, P(C.c_int32), P(C.c_int64), P(C.c_float), P(C.c_uint32)
    table = [f32, C.c_size_t, C.c_int, C.c_int, C.c_int]   # noise, count, kind, hidden, n_out
    for name, args in (("reserve", [h, C.c_int]), ("build", [h, C.c_int, i32, i64, f32]),
                       ("eval", [h, C.c_int, i32, i64, f32, u32, C.c_int, f32, f32, i32]), ("promote", [h, C.c_int, i32, i64, f32]),
                       ("parents", [h]), ("get_parent", [h, C.c_int, f32]), ("colscale_host", table + [C.c_int64, f32]),
                       ("theta_host", table + [i64, f32, C.c_int, f32]), ("members_host", table + [f32, C.c_int, i32, i64, f32, C.c_int, f32])):
        fn = getattr(lib, "dne_mujoco_ga_" + name)
        fn.argtypes, fn.restype = args, C.c_int


def num_params(kind, nact=18):
    return load().dne_num_params(int(kind), int(nact))


class PlanFacts(C.Structure):
    _fields_ = [("dense_scale", C.c_double)] + \
               [(n, C.c_int32) for n in ("kind", "members_materialized", "uniform_base", "antithetic_slot0", "pair_sigma_uniform", "n_streams",
                                         "has_y3s", "has_theta_perm", "has_scaled_table")] + [("reserved", C.c_int32 * 3)]


class WindowPlan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("lo", "cnt", "wide", "skip", "conv", "s1", "s2", "act2", "fc", "sub_spw", "sub_blocks", "solo", "sweep",
                                         "fat", "ring_scaled", "tail", "spec", "head_fused", "render_fused", "render_bands", "render_wg",
                                         "chain")] + [("reserved", C.c_int32 * 2)]


CONV_NAMES = ("lconv", "k_conv12", "k_conv12t", "split")                                  # DNE_CONV_*
FC_NAMES = ("k_lfc_cols", "k_lfc", "k_fc_sub", "k_fc_quad", "k_fc_tail", "k_fc_cols", "k_fc_ring", "k_fc_duo", "k_fc2", "k_fc", "k_lfc_pair")   # DNE_FC_*


def debug_plan(kind, nact, total, gsize, whole_eval=False, **facts):
    """dne_debug_plan (no GPU needed): the windows of a burst that starts with `total` active groups, knobs from the environment.  facts: the
    fields of PlanFacts (default: four streams, dense_scale 1, nothing else).  Returns the list of WindowPlan rows, or with whole_eval the
    evaluation's fc_full_kind."""
    f = PlanFacts(dense_scale=1.0, n_streams=4)
    for k, v in facts.items():
        setattr(f, k, v)
    rows, nsub = (WindowPlan * 4)(), C.c_int(0)
    rc = load().dne_debug_plan(int(kind), int(nact), C.byref(f), int(total), int(gsize), rows, 4, C.byref(nsub), int(bool(whole_eval)))
    if rc < 0:
        raise DneError(load().dne_last_error(None).decode())
    return rc if whole_eval else list(rows[:nsub.value])


def debug_plan_act(kind, nact, n, **facts):
    """dne_debug_plan_act (no GPU needed): the one WindowPlan row of dne_act / dne_env_step over n members, knobs from the environment"""
    f = PlanFacts(dense_scale=1.0, n_streams=4)
    for k, v in facts.items():
        setattr(f, k, v)
    row = WindowPlan()
    if load().dne_debug_plan_act(int(kind), int(nact), C.byref(f), int(n), C.byref(row)) != 0:
        raise DneError(load().dne_last_error(None).decode())
    return row


def debug_knob(kind, nact, name):
    """the value dne_create would read for one DNE_* knob under the current environment (-1: no such knob)"""
    return load().dne_debug_knob(int(kind), int(nact), name.encode())


def debug_out_head(kind, gsize, nact, noise, base, off, scale, sums, y3, actions, logits=None, bn=None, done=None, list=None, sub_sums=False,
                   reserve_lds_kb=0):
    """dne_debug_out_head: k_out (the policy head behind the streaming fc kernels) on arrays the caller lays out, 1 .. 32 actions.  y3 [n][256]
    float32, actions [n] int32 and logits [n][nact] float32 (or None) are read and overwritten in place, so what the kernel did not write keeps
    the caller's values.  sums: [n][4][256], or [n][32][256] with sub_sums.  list: group indices (None: every group in order)."""
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    noise, base, scale, sums, bn = f32(noise), f32(base), f32(scale), f32(sums), f32(bn)
    off = np.ascontiguousarray(off, np.int64)
    done = None if done is None else np.ascontiguousarray(done, np.int32)
    list = None if list is None else np.ascontiguousarray(list, np.int32)
    n = off.size
    assert y3.dtype == np.float32 and y3.shape == (n, 256) and y3.flags.c_contiguous and actions.dtype == np.int32 and actions.shape == (n,)
    assert logits is None or (logits.dtype == np.float32 and logits.shape == (n, nact) and logits.flags.c_contiguous)
    assert sums.shape == (n, 32 if sub_sums else 4, 256) and scale.shape == (n,) and (bn is None or bn.shape == (n, 608))
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))
    fn = load().dne_debug_out_head
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_int64),
                   C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float),
                   C.POINTER(C.c_int32), C.POINTER(C.c_float)]
    rc = fn(int(kind), int(gsize), int(nact), n, p(list, C.c_int32), n // gsize if list is None else list.size, p(noise, C.c_float), noise.size,
            p(base, C.c_float), p(off, C.c_int64), p(scale, C.c_float), p(done, C.c_int32), p(bn, C.c_float), p(sums, C.c_float), int(bool(sub_sums)),
            int(reserve_lds_kb), p(y3, C.c_float), p(actions, C.c_int32), p(logits, C.c_float))
    if rc != 0:
        raise DneError("dne_debug_out_head refused its arguments or a HIP call failed (rc %d)" % rc)


def load_maze(path):
    """A maze file of the reference (maze.h:468-495: disable, steps, number of lines, start x y, heading, goal x y, poi x y, then the lines)
    -> (header8 float32 [8] = disable, steps, start x, start y, heading, goal x, goal y, 0; lines float32 [n][4]).  The point of interest
    feeds a radar the policy never observes and is dropped."""
    with open(path) as f:
        tok = f.read().split()
    if len(tok) < 10:
        raise DneError("%s: not a maze file (%d numbers)" % (path, len(tok)))
    vals = [float(t) for t in tok]
    n = int(vals[2])
    if n < 1 or len(vals) != 10 + 4 * n:
        raise DneError("%s: announces %d lines and holds %d numbers (10 + 4 per line expected)" % (path, n, len(vals)))
    header = np.array([vals[0], vals[1], vals[3], vals[4], vals[5], vals[6], vals[7], 0.0], np.float32)
    return header, np.array(vals[10:], np.float32).reshape(n, 4)


def _maze_args(header, lines):
    header = _arr(header, np.float32).reshape(-1); lines = _arr(lines, np.float32).reshape(-1, 4)
    if header.size != 8:
        raise DneError("maze header: 8 floats expected, got %d" % header.size)
    return header, lines


def debug_ref_index(ref):
    """dne_debug_ref_index (no GPU needed): the reference batch [F][84][84][4] u8 as unique convolution operands, as dne_set_ref_batch
    builds it.  Returns (idx1 [F][441], patches [U1][256] u8, idx2 [F][121], windows [U2][16], dedup route taken on the default knobs)."""
    ref = np.ascontiguousarray(ref, dtype=np.uint8)
    assert ref.ndim == 4 and ref.shape[1:] == OB_SHAPE
    F = ref.shape[0]
    idx1, idx2 = np.empty((F, 441), np.int32), np.empty((F, 121), np.int32)
    patches, windows = np.empty((F * 441, 256), np.uint8), np.empty((F * 121, 16), np.int32)
    u1, u2 = C.c_int(0), C.c_int(0)
    rc = load().dne_debug_ref_index(ref.ctypes.data_as(C.POINTER(C.c_uint8)), int(F), idx1.ctypes.data_as(C.POINTER(C.c_int32)),
                                    patches.ctypes.data_as(C.POINTER(C.c_uint8)), int(F * 441), idx2.ctypes.data_as(C.POINTER(C.c_int32)),
                                    windows.ctypes.data_as(C.POINTER(C.c_int32)), int(F * 121), C.byref(u1), C.byref(u2))
    if rc < 0:
        raise DneError(load().dne_last_error(None).decode())
    return idx1, patches[:u1.value].copy(), idx2, windows[:u2.value].copy(), bool(rc)


def _ck_host(rc):
    if rc != 0:
        raise DneError(load().dne_last_error(None).decode())


def maze_rollout_host(theta, header, lines, tslimit=MAZE_STEPS, want_trace=False):
    """dne_maze_rollout_host: csrc/maze.h on the CPU (no GPU, no handle) for thetas [n][498] -> returns [n], lengths [n], final xy [n][2]
    (+ trace [n][tslimit][16] with want_trace: the observation after each step, then x, y, heading, speed, ang_vel; rows past the length are 0)"""
    theta = _arr(theta, np.float32).reshape(-1, 498)
    header, lines = _maze_args(header, lines)
    n = theta.shape[0]
    ret = np.empty(n, np.float32); ln = np.empty(n, np.int32); xy = np.empty((n, 2), np.float32)
    trace = np.zeros((n, int(tslimit), MAZE_TRACE_W), np.float32) if want_trace else None
    _ck_host(load().dne_maze_rollout_host(_ptr(theta, C.c_float), n, _ptr(header, C.c_float), _ptr(lines, C.c_float), int(lines.shape[0]),
                                          int(tslimit), _ptr(ret, C.c_float), _ptr(ln, C.c_int32), _ptr(xy, C.c_float), _ptr(trace, C.c_float)))
    return (ret, ln, xy, trace) if want_trace else (ret, ln, xy)


def maze_actions_host(actions, header, lines):
    """dne_maze_actions_host: the environment alone under open-loop actions [n][T][2] -> (rows [n][T][18] = obs[11], x, y, heading, speed,
    ang_vel, collisions, reward after each step; obs0 [n][11] after reset)"""
    actions = _arr(actions, np.float32)
    n, T = actions.shape[0], actions.shape[1]
    header, lines = _maze_args(header, lines)
    rows = np.empty((n, T, 18), np.float32); obs0 = np.empty((n, MAZE_OBS), np.float32)
    _ck_host(load().dne_maze_actions_host(_ptr(actions, C.c_float), n, T, _ptr(header, C.c_float), _ptr(lines, C.c_float), int(lines.shape[0]),
                                          _ptr(rows, C.c_float), _ptr(obs0, C.c_float)))
    return rows, obs0


def maze_forward_host(theta, obs):
    """dne_maze_forward_host: the policy alone, thetas [n][498] on observations [n][11] -> (h1 [n][16], h2 [n][16], out [n][2])"""
    theta = _arr(theta, np.float32).reshape(-1, 498); obs = _arr(obs, np.float32).reshape(-1, MAZE_OBS)
    n = theta.shape[0]
    assert obs.shape[0] == n
    h1 = np.empty((n, 16), np.float32); h2 = np.empty((n, 16), np.float32); out = np.empty((n, 2), np.float32)
    _ck_host(load().dne_maze_forward_host(_ptr(theta, C.c_float), _ptr(obs, C.c_float), n, _ptr(h1, C.c_float), _ptr(h2, C.c_float), _ptr(out, C.c_float)))
    return h1, h2, out


def maze_math_host(fn, x):
    """dne_maze_math_host: csrc/maze.h's trigonometry on the CPU for doubles x [n] -> [n][2] doubles.  fn 0 sincos_d -> (sin, cos); 1 atan_d ->
    (atan, 0); 2 float degrees -> to_rad_f -> sincos_f; 3 float quotient ty / tx -> the radar's angle in degrees (tx > 0, tx < 0)"""
    x = _arr(x, np.float64).reshape(-1)
    out = np.empty((x.size, 2), np.float64)
    _ck_host(load().dne_maze_math_host(int(fn), _ptr(x, C.c_double), int(x.size), _ptr(out, C.c_double)))
    return out


def maze_novelty_host(xy, archive, k):
    """dne_maze_novelty_host: csrc/maze_novelty.h on the CPU (no GPU, no handle) for points xy [n][2] against archive [narch][2] -> float64 [n]"""
    xy = _arr(xy, np.float32).reshape(-1, 2); archive = _arr(archive, np.float32).reshape(-1, 2)
    out = np.empty(xy.shape[0], np.float64)
    _ck_host(load().dne_maze_novelty_host(_ptr(xy, C.c_float), int(xy.shape[0]), _ptr(archive, C.c_float), int(archive.shape[0]), int(k),
                                          _ptr(out, C.c_double)))
    return out


def maze_novelty_pool_host(xy, archive, k):
    """dne_maze_novelty_pool_host: csrc/maze_novelty.h's pool form on the CPU (no GPU, no handle): each of the points xy [n][2] against the
    archive [narch][2] (None or empty: no archive) and the other n - 1 points -> float64 [n]"""
    xy = _arr(xy, np.float32).reshape(-1, 2)
    archive = _arr(np.zeros((0, 2)) if archive is None else archive, np.float32).reshape(-1, 2)
    out = np.empty(xy.shape[0], np.float64)
    _ck_host(load().dne_maze_novelty_pool_host(_ptr(xy, C.c_float), int(xy.shape[0]), _ptr(archive, C.c_float) if archive.size else None,
                                               int(archive.shape[0]), int(k), _ptr(out, C.c_double)))
    return out


def split_genome(genome):
    """a gpu-tree genome (idx0, (idx1, power1), ...) -- the root as a bare index or a 1-tuple -- as (int64 indices, float32 powers); the root's power is 0"""
    idx = np.array([c[0] if isinstance(c, (tuple, list)) else c for c in genome], np.int64)
    pw = np.array([c[1] if isinstance(c, (tuple, list)) and len(c) > 1 else 0.0 for c in genome], np.float32)
    return idx, pw


def _maze_ga_members(parent, idx, power):
    parent = _arr(parent, np.int32).reshape(-1); idx = _arr(idx, np.int64).reshape(-1)
    power = _arr(np.broadcast_to(np.asarray(power, np.float32), parent.shape), np.float32)
    if idx.size != parent.size:
        raise DneError("member descriptors: %d parents, %d indices" % (parent.size, idx.size))
    return parent, idx, power


def maze_ga_theta_host(noise, scale_by, genome):
    """dne_maze_ga_theta_host: csrc/maze_ga.h on the CPU (no GPU, no handle): theta [498] of one genome (idx0, (idx1, power1), ...)"""
    noise = _arr(noise, np.float32).reshape(-1); scale_by = _arr(scale_by, np.float32).reshape(-1)
    if scale_by.size != 498:
        raise DneError("maze_ga_theta_host: scale_by holds %d values, 498 expected" % scale_by.size)
    idx, pw = split_genome(genome)
    out = np.empty(498, np.float32)
    _ck_host(load().dne_maze_ga_theta_host(_ptr(noise, C.c_float), C.c_size_t(noise.size), _ptr(scale_by, C.c_float), _ptr(idx, C.c_int64),
                                           _ptr(pw, C.c_float), int(idx.size), _ptr(out, C.c_float)))
    return out


def maze_ga_members_host(noise, scale_by, bank, parent, idx, power):
    """dne_maze_ga_members_host: the theta [n][498] of n member descriptors (parent, idx, power) against a host bank [T][498] (None: empty):
    parent -1 a root, idx < 0 the parent itself, otherwise bank[parent] + fl(power * noise[idx:idx + 498])"""
    noise = _arr(noise, np.float32).reshape(-1); scale_by = _arr(scale_by, np.float32).reshape(-1)
    if scale_by.size != 498:
        raise DneError("maze_ga_members_host: scale_by holds %d values, 498 expected" % scale_by.size)
    bank = np.zeros((0, 498), np.float32) if bank is None else _arr(bank, np.float32).reshape(-1, 498)
    parent, idx, power = _maze_ga_members(parent, idx, power)
    out = np.empty((parent.size, 498), np.float32)
    _ck_host(load().dne_maze_ga_members_host(_ptr(noise, C.c_float), C.c_size_t(noise.size), _ptr(scale_by, C.c_float),
                                             _ptr(bank, C.c_float) if bank.shape[0] else None, int(bank.shape[0]), _ptr(parent, C.c_int32),
                                             _ptr(idx, C.c_int64), _ptr(power, C.c_float), int(parent.size), _ptr(out, C.c_float)))
    return out


def cartpole_reset_host(seed):
    """dne_cartpole_reset_host: the reset state (x, x_dot, theta, theta_dot) of one uint32 environment seed, float64 [4]"""
    out = np.empty(4, np.float64)
    _ck_host(load().dne_cartpole_reset_host(C.c_uint32(int(seed)), _ptr(out, C.c_double)))
    return out


def cartpole_rollout_host(theta, seeds, tslimit=CARTPOLE_STEPS, init=None, want_trace=False):
    """dne_cartpole_rollout_host: csrc/cartpole.h on the CPU (no GPU, no handle) for thetas [n][386] under environment seeds [n] (init [n][4]:
    explicit initial states instead) -> returns [n], lengths [n], final states float64 [n][4] (, trace float64 [n][tslimit][8] = the
    observation after each step as doubles, then the state; rows past an episode's length stay zero)"""
    theta = _arr(theta, np.float32).reshape(-1, CARTPOLE_P)
    n = theta.shape[0]
    seeds = _arr(seeds, np.uint32).reshape(-1)
    if seeds.size != n:
        raise DneError("cartpole_rollout_host: %d thetas, %d seeds" % (n, seeds.size))
    if init is not None:
        init = _arr(init, np.float64).reshape(-1, 4)
        if init.shape[0] != n:
            raise DneError("cartpole_rollout_host: %d thetas, %d initial states" % (n, init.shape[0]))
    ret = np.empty(n, np.float32); ln = np.empty(n, np.int32); state = np.empty((n, 4), np.float64)
    trace = np.zeros((n, int(tslimit), CARTPOLE_TRACE_W), np.float64) if want_trace else None
    _ck_host(load().dne_cartpole_rollout_host(_ptr(theta, C.c_float), n, _ptr(seeds, C.c_uint32), _ptr(init, C.c_double), int(tslimit),
                                              _ptr(ret, C.c_float), _ptr(ln, C.c_int32), _ptr(state, C.c_double), _ptr(trace, C.c_double)))
    return (ret, ln, state, trace) if want_trace else (ret, ln, state)


def cartpole_actions_host(actions, init):
    """dne_cartpole_actions_host: the environment alone under open-loop actions [n][T] (0 / 1) from initial states [n][4] -> rows float64
    [n][T][5] = the state after each step, then done (1 / 0); the stepping goes on past done"""
    actions = _arr(actions, np.int32); actions = actions.reshape(-1, actions.shape[-1])
    n, T = actions.shape
    init = _arr(init, np.float64).reshape(-1, 4)
    if init.shape[0] != n:
        raise DneError("cartpole_actions_host: %d sequences, %d initial states" % (n, init.shape[0]))
    rows = np.empty((n, T, 5), np.float64)
    _ck_host(load().dne_cartpole_actions_host(_ptr(actions, C.c_int32), n, T, _ptr(init, C.c_double), _ptr(rows, C.c_double)))
    return rows


def cartpole_forward_host(theta, obs):
    """dne_cartpole_forward_host: the policy alone, thetas [n][386] on observations [n][4] -> (h1 [n][16], h2 [n][16], out [n][2])"""
    theta = _arr(theta, np.float32).reshape(-1, CARTPOLE_P); obs = _arr(obs, np.float32).reshape(-1, CARTPOLE_OBS)
    n = theta.shape[0]
    if obs.shape[0] != n:
        raise DneError("cartpole_forward_host: %d thetas, %d observations" % (n, obs.shape[0]))
    h1 = np.empty((n, 16), np.float32); h2 = np.empty((n, 16), np.float32); out = np.empty((n, 2), np.float32)
    _ck_host(load().dne_cartpole_forward_host(_ptr(theta, C.c_float), _ptr(obs, C.c_float), n, _ptr(h1, C.c_float), _ptr(h2, C.c_float), _ptr(out, C.c_float)))
    return h1, h2, out


def pendulum_num_params(hidden, n_out=1):
    """dne_pendulum_num_params: P = 5 H + H^2 + H O + O (-1: a width or an output count csrc/pendulum.h does not build)"""
    return load().dne_pendulum_num_params(int(hidden), int(n_out))


def pendulum_reset_host(seed):
    """dne_pendulum_reset_host: the reset state (theta, theta_dot) of one uint32 environment seed, float64 [2]"""
    out = np.empty(2, np.float64)
    _ck_host(load().dne_pendulum_reset_host(C.c_uint32(int(seed)), _ptr(out, C.c_double)))
    return out


def _pendulum_shape(hidden, n_out, ac_mode, nonlin):
    return int(hidden), int(n_out), int(PENDULUM_AC_MODES.get(ac_mode, ac_mode)), int(PENDULUM_NONLINS.get(nonlin, nonlin))


def pendulum_rollout_host(theta, seeds, hidden, mean, std, n_out=1, ac_mode='continuous', nonlin='tanh', tslimit=PENDULUM_STEPS, init=None,
                          ac_noise_std=0.0, table=None, ac_off=None, stat_flag=None, want_trace=False):
    """dne_pendulum_rollout_host: csrc/pendulum.h on the CPU (no GPU, no handle) for thetas [n][P] under environment seeds [n] (init [n][2]:
    explicit initial states instead).  table / ac_off [n] (both or neither): the noise table and where each member's 200 action-noise values
    start (< 0: none); stat_flag [n]: who accumulates its observations.  -> dict(returns, signreturns, lengths, state [n][2], ob_sum [n][3],
    ob_sumsq [n][3], ob_count [n](, trace float64 [n][tslimit][8]: the three observations acted on, the net's action, the action applied,
    the reward, theta and theta_dot after the step))"""
    hidden, n_out, ac_mode, nonlin = _pendulum_shape(hidden, n_out, ac_mode, nonlin)
    P = pendulum_num_params(hidden, n_out)
    if P < 0:
        raise DneError("pendulum_rollout_host: hidden width %d with %d outputs is not a shape csrc/pendulum.h builds" % (hidden, n_out))
    theta = _arr(theta, np.float32).reshape(-1, P)
    n = theta.shape[0]
    seeds = _arr(seeds, np.uint32).reshape(-1)
    if seeds.size != n:
        raise DneError("pendulum_rollout_host: %d thetas, %d seeds" % (n, seeds.size))
    mean = _arr(mean, np.float32).reshape(3); std = _arr(std, np.float32).reshape(3)
    if init is not None:
        init = _arr(init, np.float64).reshape(-1, 2)
        if init.shape[0] != n:
            raise DneError("pendulum_rollout_host: %d thetas, %d initial states" % (n, init.shape[0]))
    if table is not None:
        table = _arr(table, np.float32).reshape(-1)
    if ac_off is not None:
        ac_off = _arr(ac_off, np.int64).reshape(-1)
        if ac_off.size != n:
            raise DneError("pendulum_rollout_host: %d thetas, %d action-noise offsets" % (n, ac_off.size))
    if stat_flag is not None:
        stat_flag = _arr(stat_flag, np.uint8).reshape(-1)
        if stat_flag.size != n:
            raise DneError("pendulum_rollout_host: %d thetas, %d statistics flags" % (n, stat_flag.size))
    r = dict(returns=np.empty(n, np.float32), signreturns=np.empty(n, np.float32), lengths=np.empty(n, np.int32), state=np.empty((n, 2), np.float64),
             ob_sum=np.empty((n, 3), np.float64), ob_sumsq=np.empty((n, 3), np.float64), ob_count=np.empty(n, np.int32))
    trace = np.zeros((n, int(tslimit), PENDULUM_TRACE_W), np.float64) if want_trace else None
    _ck_host(load().dne_pendulum_rollout_host(
        _ptr(theta, C.c_float), n, hidden, n_out, ac_mode, nonlin, _ptr(mean, C.c_float), _ptr(std, C.c_float), _ptr(seeds, C.c_uint32),
        _ptr(init, C.c_double), int(tslimit), C.c_float(ac_noise_std), _ptr(table, C.c_float), C.c_size_t(0 if table is None else table.size),
        _ptr(ac_off, C.c_int64), _ptr(stat_flag, C.c_uint8), _ptr(r['returns'], C.c_float), _ptr(r['signreturns'], C.c_float),
        _ptr(r['lengths'], C.c_int32), _ptr(r['state'], C.c_double), _ptr(r['ob_sum'], C.c_double), _ptr(r['ob_sumsq'], C.c_double),
        _ptr(r['ob_count'], C.c_int32), _ptr(trace, C.c_double)))
    if want_trace:
        r['trace'] = trace
    return r


def pendulum_actions_host(actions, init):
    """dne_pendulum_actions_host: the environment alone under open-loop float actions [n][T] from initial states [n][2] -> rows float64
    [n][T][3] = theta and theta_dot after each step, then the reward"""
    actions = _arr(actions, np.float32); actions = actions.reshape(-1, actions.shape[-1])
    n, T = actions.shape
    init = _arr(init, np.float64).reshape(-1, 2)
    if init.shape[0] != n:
        raise DneError("pendulum_actions_host: %d sequences, %d initial states" % (n, init.shape[0]))
    rows = np.empty((n, T, 3), np.float64)
    _ck_host(load().dne_pendulum_actions_host(_ptr(actions, C.c_float), n, T, _ptr(init, C.c_double), _ptr(rows, C.c_double)))
    return rows


def pendulum_forward_host(theta, obs, hidden, mean, std, n_out=1, ac_mode='continuous', nonlin='tanh'):
    """dne_pendulum_forward_host: the policy alone, thetas [n][P] on raw observations [n][3] -> (x [n][3] normalised and clipped, h1 [n][H],
    h2 [n][H], out [n][O], action [n])"""
    hidden, n_out, ac_mode, nonlin = _pendulum_shape(hidden, n_out, ac_mode, nonlin)
    P = pendulum_num_params(hidden, n_out)
    if P < 0:
        raise DneError("pendulum_forward_host: hidden width %d with %d outputs is not a shape csrc/pendulum.h builds" % (hidden, n_out))
    theta = _arr(theta, np.float32).reshape(-1, P); obs = _arr(obs, np.float32).reshape(-1, PENDULUM_OBS)
    n = theta.shape[0]
    if obs.shape[0] != n:
        raise DneError("pendulum_forward_host: %d thetas, %d observations" % (n, obs.shape[0]))
    mean = _arr(mean, np.float32).reshape(3); std = _arr(std, np.float32).reshape(3)
    x = np.empty((n, 3), np.float32); h1 = np.empty((n, hidden), np.float32); h2 = np.empty((n, hidden), np.float32)
    out = np.empty((n, n_out), np.float32); action = np.empty(n, np.float32)
    _ck_host(load().dne_pendulum_forward_host(_ptr(theta, C.c_float), _ptr(obs, C.c_float), n, hidden, n_out, ac_mode, nonlin, _ptr(mean, C.c_float),
                                              _ptr(std, C.c_float), _ptr(x, C.c_float), _ptr(h1, C.c_float), _ptr(h2, C.c_float), _ptr(out, C.c_float),
                                              _ptr(action, C.c_float)))
    return x, h1, h2, out, action


def mjmaze_num_params(hidden, n_out=2):
    """dne_mjmaze_num_params: P = 13 H + H^2 + H O + O (-1: a width or an output count csrc/mjmaze.h does not build)"""
    return load().dne_mjmaze_num_params(int(hidden), int(n_out))


def mjmaze_rollout_host(theta, header, lines, hidden, mean, std, n_out=2, ac_mode='continuous', nonlin='tanh', tslimit=MJMAZE_STEPS,
                        ac_noise_std=0.0, table=None, ac_off=None, stat_flag=None, want_trace=False):
    """dne_mjmaze_rollout_host: csrc/mjmaze.h on the CPU (no GPU, no handle) for thetas [n][P] in the maze (header [8], lines [w][4]).
    table / ac_off [n] (both or neither): the noise table and where each member's 800 action-noise values start (< 0: none); stat_flag [n]: who
    accumulates its observations.  -> dict(returns, signreturns, lengths, xy [n][2], ob_sum [n][11], ob_sumsq [n][11], ob_count [n](, trace
    float32 [n][tslimit][20]: the 11 observations acted on, the net's 2 actions, the 2 applied, x, y, heading, speed, ang_vel after the step))"""
    hidden, n_out, ac_mode, nonlin = _pendulum_shape(hidden, n_out, ac_mode, nonlin)
    P = mjmaze_num_params(hidden, n_out)
    if P < 0:
        raise DneError("mjmaze_rollout_host: hidden width %d with %d outputs is not a shape csrc/mjmaze.h builds" % (hidden, n_out))
    theta = _arr(theta, np.float32).reshape(-1, P)
    n = theta.shape[0]
    header, lines = _maze_args(header, lines)
    mean = _arr(mean, np.float32).reshape(MJMAZE_OBS); std = _arr(std, np.float32).reshape(MJMAZE_OBS)
    if table is not None:
        table = _arr(table, np.float32).reshape(-1)
    if ac_off is not None:
        ac_off = _arr(ac_off, np.int64).reshape(-1)
        if ac_off.size != n:
            raise DneError("mjmaze_rollout_host: %d thetas, %d action-noise offsets" % (n, ac_off.size))
    if stat_flag is not None:
        stat_flag = _arr(stat_flag, np.uint8).reshape(-1)
        if stat_flag.size != n:
            raise DneError("mjmaze_rollout_host: %d thetas, %d statistics flags" % (n, stat_flag.size))
    r = dict(returns=np.empty(n, np.float32), signreturns=np.empty(n, np.float32), lengths=np.empty(n, np.int32), xy=np.empty((n, 2), np.float32),
             ob_sum=np.empty((n, MJMAZE_OBS), np.float64), ob_sumsq=np.empty((n, MJMAZE_OBS), np.float64), ob_count=np.empty(n, np.int32))
    trace = np.zeros((n, int(tslimit), MJMAZE_TRACE_W), np.float32) if want_trace else None
    _ck_host(load().dne_mjmaze_rollout_host(
        _ptr(theta, C.c_float), n, hidden, n_out, ac_mode, nonlin, _ptr(mean, C.c_float), _ptr(std, C.c_float), _ptr(header, C.c_float),
        _ptr(lines, C.c_float), int(lines.shape[0]), int(tslimit), C.c_float(ac_noise_std), _ptr(table, C.c_float),
        C.c_size_t(0 if table is None else table.size), _ptr(ac_off, C.c_int64), _ptr(stat_flag, C.c_uint8), _ptr(r['returns'], C.c_float),
        _ptr(r['signreturns'], C.c_float), _ptr(r['lengths'], C.c_int32), _ptr(r['xy'], C.c_float), _ptr(r['ob_sum'], C.c_double),
        _ptr(r['ob_sumsq'], C.c_double), _ptr(r['ob_count'], C.c_int32), _ptr(trace, C.c_float)))
    if want_trace:
        r['trace'] = trace
    return r


def mjmaze_forward_host(theta, obs, hidden, mean, std, n_out=2, ac_mode='continuous', nonlin='tanh'):
    """dne_mjmaze_forward_host: the policy alone, thetas [n][P] on raw observations [n][11] -> (x [n][11] normalised and clipped, h1 [n][H],
    h2 [n][H], out [n][O], action [n][2])"""
    hidden, n_out, ac_mode, nonlin = _pendulum_shape(hidden, n_out, ac_mode, nonlin)
    P = mjmaze_num_params(hidden, n_out)
    if P < 0:
        raise DneError("mjmaze_forward_host: hidden width %d with %d outputs is not a shape csrc/mjmaze.h builds" % (hidden, n_out))
    theta = _arr(theta, np.float32).reshape(-1, P); obs = _arr(obs, np.float32).reshape(-1, MJMAZE_OBS)
    n = theta.shape[0]
    if obs.shape[0] != n:
        raise DneError("mjmaze_forward_host: %d thetas, %d observations" % (n, obs.shape[0]))
    mean = _arr(mean, np.float32).reshape(MJMAZE_OBS); std = _arr(std, np.float32).reshape(MJMAZE_OBS)
    x = np.empty((n, MJMAZE_OBS), np.float32); h1 = np.empty((n, hidden), np.float32); h2 = np.empty((n, hidden), np.float32)
    out = np.empty((n, n_out), np.float32); action = np.empty((n, MJMAZE_ADIM), np.float32)
    _ck_host(load().dne_mjmaze_forward_host(_ptr(theta, C.c_float), _ptr(obs, C.c_float), n, hidden, n_out, ac_mode, nonlin, _ptr(mean, C.c_float),
                                            _ptr(std, C.c_float), _ptr(x, C.c_float), _ptr(h1, C.c_float), _ptr(h2, C.c_float), _ptr(out, C.c_float),
                                            _ptr(action, C.c_float)))
    return x, h1, h2, out, action


def pendulum_math_host(fn, x, a=0.0, b=1.0):
    """dne_pendulum_math_host: 'tanh' -> tanh_f(float32(x)), 'norm' -> norm_angle(x), 'normalise' -> clip((float32(x) - a) / b, -5, 5); float64 in and out"""
    x = _arr(x, np.float64).reshape(-1)
    out = np.empty(x.size, np.float64)
    _ck_host(load().dne_pendulum_math_host(int(PENDULUM_MATH.get(fn, fn)), _ptr(x, C.c_double), int(x.size), C.c_float(a), C.c_float(b), _ptr(out, C.c_double)))
    return out


STEPENV_KINDS = (KIND_MAZE, KIND_CARTPOLE, KIND_PENDULUM)   # the engine kinds that step their own environment (csrc/step_env.h)
STEP_ENVS = STEPENV_KINDS + (ENV_ACROBOT,)                  # every id that has a step environment: those kinds, and the environments a KIND_DENSE engine alone steps


def stepenv_dims(kind):
    """dne_stepenv_dims: (observation width, action width, state doubles, actions are int32) of a kind; DneError for a kind without such an
    environment"""
    v = [C.c_int(0) for _ in range(4)]
    _ck_host(load().dne_stepenv_dims(int(kind), *[C.byref(x) for x in v]))
    return v[0].value, v[1].value, v[2].value, bool(v[3].value)


def acrobot_actions_host(actions, init):
    """dne_acrobot_actions_host: the acrobot alone under open-loop actions [n][T] (0 / 1 / 2) from initial states [n][4] -> rows float64
    [n][T][5] = the state after each step, then terminal (1 / 0); the stepping goes on past it"""
    actions = _arr(actions, np.int32); actions = actions.reshape(-1, actions.shape[-1])
    n, T = actions.shape
    init = _arr(init, np.float64).reshape(-1, 4)
    if init.shape[0] != n:
        raise DneError("acrobot_actions_host: %d sequences, %d initial states" % (n, init.shape[0]))
    rows = np.empty((n, T, 5), np.float64)
    _ck_host(load().dne_acrobot_actions_host(_ptr(actions, C.c_int32), n, T, _ptr(init, C.c_double), _ptr(rows, C.c_double)))
    return rows


def _stepenv_maze(kind, header, lines):
    """(header pointer, lines pointer, n_walls, the arrays kept alive) for a host twin: the maze's, NULL / NULL / 0 for the other kinds"""
    if int(kind) != KIND_MAZE:
        return None, None, 0, ()
    if header is None or lines is None:
        raise DneError("stepenv: the maze's host twin needs header and lines (load_maze)")
    header, lines = _maze_args(header, lines)
    return _ptr(header, C.c_float), _ptr(lines, C.c_float), int(lines.shape[0]), (header, lines)


def stepenv_reset_host(kind, n, seeds=None, max_steps=0, header=None, lines=None):
    """dne_stepenv_reset_host: n environments of `kind` after reset -> (state float64 [n][S], steps int32 [n], limit int32 [n], done uint8 [n],
    obs float32 [n][OBS]).  seeds uint32 [n] (the maze reads none); max_steps <= 0: the environment's own limit."""
    obs_w, _, S, _ = stepenv_dims(kind)
    n = int(n)
    if seeds is not None:
        seeds = _arr(seeds, np.uint32).reshape(-1)
        if seeds.size != n:
            raise DneError("stepenv_reset_host: %d environments, %d seeds" % (n, seeds.size))
    hp, lp, nw, _keep = _stepenv_maze(kind, header, lines)
    state = np.empty((max(n, 0), S), np.float64); steps = np.empty(max(n, 0), np.int32); limit = np.empty(max(n, 0), np.int32)
    done = np.empty(max(n, 0), np.uint8); obs = np.empty((max(n, 0), obs_w), np.float32)
    _ck_host(load().dne_stepenv_reset_host(int(kind), n, _ptr(seeds, C.c_uint32), hp, lp, nw, int(max_steps), _ptr(state, C.c_double),
                                           _ptr(steps, C.c_int32), _ptr(limit, C.c_int32), _ptr(done, C.c_uint8), _ptr(obs, C.c_float)))
    return state, steps, limit, done, obs


def _stepenv_actions(kind, actions, n):
    """the actions of one step as the C ABI takes them: float32 [n][2] (maze), int32 [n] (cart-pole, acrobot), float32 [n] (pendulum)"""
    _, act_w, _, is_int = stepenv_dims(kind)
    a = _arr(actions, np.int32 if is_int else np.float32).reshape(-1)
    if a.size != n * act_w:
        raise DneError("stepenv: %d environments take %d action values, %d given" % (n, n * act_w, a.size))
    return a, is_int


def stepenv_step_host(kind, actions, state, steps, limit, done, obs, header=None, lines=None):
    """dne_stepenv_step_host: one step of the n environments held in (state, steps, limit, done, obs) as stepenv_reset_host returned them, IN
    PLACE -> reward float32 [n].  A done environment keeps every bit and earns 0."""
    n = steps.shape[0]
    for a, t in ((state, np.float64), (steps, np.int32), (limit, np.int32), (done, np.uint8), (obs, np.float32)):
        if a.dtype != t or not a.flags.c_contiguous:
            raise DneError("stepenv_step_host: the batch arrays are stepenv_reset_host's own (contiguous %s expected)" % np.dtype(t).name)
    a, is_int = _stepenv_actions(kind, actions, n)
    hp, lp, nw, _keep = _stepenv_maze(kind, header, lines)
    reward = np.empty(n, np.float32)
    _ck_host(load().dne_stepenv_step_host(int(kind), int(n), C.cast(_ptr(a, C.c_int32 if is_int else C.c_float), C.c_void_p), hp, lp, nw,
                                          _ptr(state, C.c_double), _ptr(steps, C.c_int32), _ptr(limit, C.c_int32), _ptr(done, C.c_uint8),
                                          _ptr(reward, C.c_float), _ptr(obs, C.c_float)))
    return reward


def stepenv_observe_host(kind, state, header=None, lines=None):
    """dne_stepenv_observe_host: the observations float32 [n][OBS] of states float64 [n][S]"""
    obs_w, _, S, _ = stepenv_dims(kind)
    state = _arr(state, np.float64).reshape(-1, S)
    hp, lp, nw, _keep = _stepenv_maze(kind, header, lines)
    obs = np.empty((state.shape[0], obs_w), np.float32)
    _ck_host(load().dne_stepenv_observe_host(int(kind), int(state.shape[0]), _ptr(state, C.c_double), hp, lp, nw, _ptr(obs, C.c_float)))
    return obs


# ---- dense policies of any small shape on the step environments (csrc/dense.h) ------------------------------------------------------------------
def _dense_shape(hidden, nonlin):
    """(n_hidden, the widths as int32 array or None, the nonlinearity's number)"""
    hidden = tuple(int(w) for w in hidden)
    return len(hidden), (np.array(hidden, np.int32) if hidden else None), int(DENSE_NONLINS.get(nonlin, nonlin))


def dense_num_params(env_kind, hidden, n_out):
    """dne_dense_num_params: P of the shape (env_kind's inputs, the hidden widths, n_out outputs), -1 for a shape that is not built"""
    L, w, _ = _dense_shape(hidden, 1)
    return load().dne_dense_num_params(int(env_kind), L, _ptr(w, C.c_int32), int(n_out))


def dense_forward_host(theta, obs, env_kind, hidden, nonlin, n_out):
    """dne_dense_forward_host: theta [n][P], obs [n][OBS] -> (layers float32 [n][sum(hidden)]: every hidden layer behind its nonlinearity, out
    float32 [n][n_out], actions as stepenv_step takes them)"""
    env_kind, n_out = int(env_kind), int(n_out)
    L, w, nl = _dense_shape(hidden, nonlin)
    obs_w, act_w, _, is_int = stepenv_dims(env_kind) if env_kind in STEP_ENVS else (1, 1, 1, False)
    P = load().dne_dense_num_params(env_kind, L, _ptr(w, C.c_int32), n_out)
    if P < 0:   # (one row of whatever was given: the call below names what is wrong with the shape)
        theta, obs = _arr(theta, np.float32).reshape(1, -1), _arr(obs, np.float32).reshape(1, -1)
    theta = _arr(theta, np.float32).reshape(-1, P if P > 0 else theta.size)
    obs = _arr(obs, np.float32).reshape(-1, obs_w if P > 0 else obs.size)
    n = theta.shape[0]
    if obs.shape[0] != n:
        raise DneError("dense_forward_host: %d thetas, %d observations" % (n, obs.shape[0]))
    layers = np.empty((n, int(sum(hidden))), np.float32); out = np.empty((n, max(n_out, 1)), np.float32)
    act = np.empty((n, act_w) if act_w > 1 else n, np.int32 if is_int else np.float32)
    _ck_host(load().dne_dense_forward_host(_ptr(theta, C.c_float), _ptr(obs, C.c_float), n, env_kind, L, _ptr(w, C.c_int32), nl, n_out,
                                           _ptr(layers, C.c_float), _ptr(out, C.c_float), C.cast(_ptr(act, C.c_int32 if is_int else C.c_float), C.c_void_p)))
    return layers, out, act


def dense_rollout_host(theta, env_kind, hidden, nonlin, n_out, seeds=None, tslimit=0, init=None, header=None, lines=None):
    """dne_dense_rollout_host: one whole episode per theta [n][P] from its reset (seeds uint32 [n]; the maze reads none) or from init [n][S], to
    the environment's own limit or tslimit (<= 0: the own limit) -> dict(returns, signreturns, lengths, state float64 [n][S])"""
    env_kind, n_out = int(env_kind), int(n_out)
    L, w, nl = _dense_shape(hidden, nonlin)
    S = stepenv_dims(env_kind)[2] if env_kind in STEP_ENVS else 1   # (another kind: the call below refuses it by name)
    P = load().dne_dense_num_params(env_kind, L, _ptr(w, C.c_int32), n_out)
    theta = _arr(theta, np.float32)
    theta = theta.reshape(-1, P) if P > 0 else theta.reshape(1, -1)   # (a shape that is not built: one row, the call below names what is wrong)
    n = theta.shape[0]
    if seeds is not None:
        seeds = _arr(seeds, np.uint32).reshape(-1)
        if seeds.size != n:
            raise DneError("dense_rollout_host: %d thetas, %d seeds" % (n, seeds.size))
    if init is not None:
        init = _arr(init, np.float64).reshape(n, S)
    if int(tslimit) <= 0:
        tslimit = {KIND_MAZE: MAZE_STEPS, KIND_CARTPOLE: CARTPOLE_STEPS, KIND_PENDULUM: PENDULUM_STEPS, ENV_ACROBOT: ACROBOT_STEPS}.get(env_kind, 1)
    hp, lp, nw, _keep = _stepenv_maze(env_kind, header, lines)
    ret = np.empty(n, np.float32); sign = np.empty(n, np.float32); ln = np.empty(n, np.int32); state = np.empty((n, S), np.float64)
    _ck_host(load().dne_dense_rollout_host(_ptr(theta, C.c_float), n, env_kind, L, _ptr(w, C.c_int32), nl, n_out, _ptr(seeds, C.c_uint32),
                                           _ptr(init, C.c_double), hp, lp, nw, int(tslimit), _ptr(ret, C.c_float), _ptr(sign, C.c_float),
                                           _ptr(ln, C.c_int32), _ptr(state, C.c_double)))
    return dict(returns=ret, signreturns=sign, lengths=ln, state=state)


# ---- Deep-GA on a dense policy (csrc/dense_ga.h): maze_ga's twins with P a parameter ---------------------------------------------------------------
def dense_ga_theta_host(noise, scale_by, genome):
    """dne_dense_ga_theta_host: csrc/dense_ga.h on the CPU (no GPU, no handle): theta [P] of one genome (idx0, (idx1, power1), ...); P is
    scale_by's length"""
    noise = _arr(noise, np.float32).reshape(-1); scale_by = _arr(scale_by, np.float32).reshape(-1)
    idx, pw = split_genome(genome)
    out = np.empty(scale_by.size, np.float32)
    _ck_host(load().dne_dense_ga_theta_host(_ptr(noise, C.c_float), C.c_size_t(noise.size), _ptr(scale_by, C.c_float), int(scale_by.size),
                                            _ptr(idx, C.c_int64), _ptr(pw, C.c_float), int(idx.size), _ptr(out, C.c_float)))
    return out


def dense_ga_members_host(noise, scale_by, bank, parent, idx, power):
    """dne_dense_ga_members_host: the theta [n][P] of n member descriptors (parent, idx, power) against a host bank [T][P] (None: empty):
    parent -1 a root, idx < 0 the parent itself, otherwise bank[parent] + fl(power * noise[idx:idx + P]); P is scale_by's length"""
    noise = _arr(noise, np.float32).reshape(-1); scale_by = _arr(scale_by, np.float32).reshape(-1)
    P = int(scale_by.size)
    bank = np.zeros((0, max(P, 1)), np.float32) if bank is None else _arr(bank, np.float32).reshape(-1, max(P, 1))
    parent, idx, power = _maze_ga_members(parent, idx, power)
    out = np.empty((parent.size, P), np.float32)
    _ck_host(load().dne_dense_ga_members_host(_ptr(noise, C.c_float), C.c_size_t(noise.size), _ptr(scale_by, C.c_float), P,
                                              _ptr(bank, C.c_float) if bank.shape[0] else None, int(bank.shape[0]), _ptr(parent, C.c_int32),
                                              _ptr(idx, C.c_int64), _ptr(power, C.c_float), int(parent.size), _ptr(out, C.c_float)))
    return out


# ---- novelty over final states on a dense policy (csrc/dense_novelty.h) ---------------------------------------------------------------------------
# ---- Deep-GA on MujocoPolicy (csrc/mujoco_ga.h): es_distributed/ga.py's genome, the root reinitialised on its noise slice -------------------------
def _mujoco_ga_table(who, noise, kind, hidden, n_out):
    kind, hidden, n_out = int(kind), int(hidden), int(n_out)
    P = pendulum_num_params(hidden, n_out) if kind == KIND_PENDULUM else mjmaze_num_params(hidden, n_out) if kind == KIND_MJMAZE else -1
    if P < 0:
        raise DneError("%s: kind %d, hidden width %d with %d outputs is not a MujocoPolicy shape csrc/pendulum.h or csrc/mjmaze.h builds" % (who, kind, hidden, n_out))
    noise = _arr(noise, np.float32).reshape(-1)
    return noise, (_ptr(noise, C.c_float), noise.size, kind, hidden, n_out), P


def mujoco_ga_colscale_host(noise, kind, hidden, n_out, idx0):
    """dne_mujoco_ga_colscale_host: the 2 H + O column scales 1 / sqrt(sum of squares) of the slice noise[idx0:idx0 + P] in the layout of `kind`
    (KIND_PENDULUM or KIND_MJMAZE): the H columns of l0/w, the H of l1/w, the O of out/w, each summed in numpy's order"""
    noise, table, P = _mujoco_ga_table("mujoco_ga_colscale_host", noise, kind, hidden, n_out)
    out = np.empty(2 * int(hidden) + int(n_out), np.float32)
    _ck_host(load().dne_mujoco_ga_colscale_host(*table, int(idx0), _ptr(out, C.c_float)))
    return out


def mujoco_ga_theta_host(noise, kind, hidden, n_out, genome):
    """dne_mujoco_ga_theta_host: csrc/mujoco_ga.h on the CPU (no GPU, no handle): theta [P] of one genome (idx0, (idx1, power1), ...) -- the
    policy reinitialised on noise[idx0:idx0 + P], then theta += fl(power_j * noise[idx_j:idx_j + P]) per further seed"""
    noise, table, P = _mujoco_ga_table("mujoco_ga_theta_host", noise, kind, hidden, n_out)
    idx, pw = split_genome(genome)
    out = np.empty(P, np.float32)
    _ck_host(load().dne_mujoco_ga_theta_host(*table, _ptr(idx, C.c_int64), _ptr(pw, C.c_float), int(idx.size), _ptr(out, C.c_float)))
    return out


def mujoco_ga_members_host(noise, kind, hidden, n_out, bank, parent, idx, power):
    """dne_mujoco_ga_members_host: the theta [n][P] of n member descriptors (parent, idx, power) against a host bank [T][P] (None: empty):
    parent -1 a root at idx, idx < 0 the parent itself, otherwise bank[parent] + fl(power * noise[idx:idx + P])"""
    noise, table, P = _mujoco_ga_table("mujoco_ga_members_host", noise, kind, hidden, n_out)
    bank = np.zeros((0, P), np.float32) if bank is None else _arr(bank, np.float32).reshape(-1, P)
    parent, idx, power = _maze_ga_members(parent, idx, power)
    out = np.empty((parent.size, P), np.float32)
    _ck_host(load().dne_mujoco_ga_members_host(*table, _ptr(bank, C.c_float) if bank.shape[0] else None, int(bank.shape[0]), _ptr(parent, C.c_int32),
                                               _ptr(idx, C.c_int64), _ptr(power, C.c_float), int(parent.size), _ptr(out, C.c_float)))
    return out


def dense_bc_dim(env_kind):
    """D of an environment's behaviour characterisation: the cart-pole 4 (x, x_dot, theta, theta_dot), the acrobot 4 (theta1, theta2, omega1,
    omega2), the maze (x, y) and the pendulum (theta, theta_dot) 2"""
    return 4 if int(env_kind) in (KIND_CARTPOLE, ENV_ACROBOT) else 2


def dense_bc_host(env_kind, rec):
    """dne_dense_bc_host: the BCs float32 [n][D] of final state records float64 [n][S] (dense_final_state's, dense_rollout_host's 'state')"""
    env_kind = int(env_kind)
    S = stepenv_dims(env_kind)[2] if env_kind in STEP_ENVS else 1   # (another kind: the call below refuses it by name)
    rec = None if rec is None else _arr(rec, np.float64).reshape(-1, S)
    n = 0 if rec is None else int(rec.shape[0])
    out = np.empty((n, dense_bc_dim(env_kind)), np.float32)
    _ck_host(load().dne_dense_bc_host(env_kind, _ptr(rec, C.c_double), n, _ptr(out, C.c_float)))
    return out


def dense_novelty_host(bc, archive, k, D=None):
    """dne_dense_novelty_host: csrc/dense_novelty.h on the CPU (no GPU, no handle) for BCs [n][D] against archive [narch][D] -> float64 [n];
    D is bc's second dimension unless given"""
    D = int(np.shape(bc)[-1] if D is None else D)
    bc = _arr(bc, np.float32).reshape(-1, max(D, 1)); archive = _arr(archive, np.float32).reshape(-1, max(D, 1))
    out = np.empty(bc.shape[0], np.float64)
    _ck_host(load().dne_dense_novelty_host(_ptr(bc, C.c_float), int(bc.shape[0]), _ptr(archive, C.c_float), int(archive.shape[0]), D, int(k),
                                           _ptr(out, C.c_double)))
    return out


def dense_novelty_pool_host(bc, archive, k, D=None):
    """dne_dense_novelty_pool_host: csrc/dense_novelty.h's pool form on the CPU (no GPU, no handle): each of the BCs [n][D] against the archive
    [narch][D] (None or empty: no archive) and the other n - 1 BCs -> float64 [n]; D is bc's second dimension unless given"""
    D = int(np.shape(bc)[-1] if D is None else D)
    bc = _arr(bc, np.float32).reshape(-1, max(D, 1))
    archive = _arr(np.zeros((0, max(D, 1))) if archive is None else archive, np.float32).reshape(-1, max(D, 1))
    out = np.empty(bc.shape[0], np.float64)
    _ck_host(load().dne_dense_novelty_pool_host(_ptr(bc, C.c_float), int(bc.shape[0]), _ptr(archive, C.c_float) if archive.size else None,
                                                int(archive.shape[0]), D, int(k), _ptr(out, C.c_double)))
    return out


def ram_novelty_pool_host(bc, archive, k, neighbours=False):
    """dne_ram_novelty_pool_host: csrc/ram_novelty.h on the CPU (no GPU, no handle): each of the RAM points uint8 [n][128] against the archive
    [narch][128] (None or empty: no archive) and the other n - 1 points -> float64 [n]; with neighbours also int32 [n][min(k, narch + n - 1)],
    each member's nearest combined slots in the contract's order"""
    bc = _arr(bc, np.uint8).reshape(-1, RAM_BYTES)
    archive = _arr(np.zeros((0, RAM_BYTES), np.uint8) if archive is None else archive, np.uint8).reshape(-1, RAM_BYTES)
    n, A = int(bc.shape[0]), int(archive.shape[0])
    out = np.empty(n, np.float64)
    nb = np.empty((n, max(min(int(k), A + n - 1), 0)), np.int32) if neighbours else None
    _ck_host(load().dne_ram_novelty_pool_host(_ptr(bc, C.c_uint8), n, _ptr(archive, C.c_uint8) if A else None, A, int(k), _ptr(out, C.c_double),
                                              _ptr(nb, C.c_int32)))
    return (out, nb) if neighbours else out


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


class Engine:
    """One engine = one GPU.  Thin, typed wrapper; every method maps 1:1 onto a dne_* entry point.

    n_actions: 2..18 (env.action_space.n).  The SynthAtari fixture defines 18 actions in ALE order; an engine with fewer uses the first
    n_actions of them, and dne_create refuses a wider one (DneError)."""

    def __init__(self, kind, n_actions=18, max_members=256, ref_count=128, device_id=0, ref_chunk=0,
                 record_bc=False, bc_max_steps=0, profile_events=False, bc_final_only=False, hidden=0, ac_mode=0, nonlin=0, env=None):
        """hidden, ac_mode, nonlin: the shape of a KIND_PENDULUM or KIND_MJMAZE engine (hidden width 64 / 128 / 256; 'continuous' or 'uniform';
        'tanh' or 'relu'), with n_actions the outputs (the pendulum: 1, or the bins; the maze: 2, or twice the bins).
        A KIND_DENSE engine: env the environment (KIND_MAZE, KIND_CARTPOLE, KIND_PENDULUM or ENV_ACROBOT), hidden the tuple of hidden widths
        (() is LinearClassifier), nonlin 'tanh' or 'relu', n_actions the outputs (2, 2, 1, 3)"""
        self.lib = load()
        self.kind, self.n_actions, self.max_members = int(kind), int(n_actions), int(max_members)
        self.ref_count = int(ref_count) if kind in ES_KINDS else 0
        self.bc_max_steps = int(bc_max_steps)
        cfg = Config(device_id=device_id, policy_kind=self.kind, n_actions=self.n_actions, max_members=self.max_members,
                     ref_count=self.ref_count, ref_chunk=ref_chunk, record_bc=int(bool(record_bc)),
                     bc_max_steps=self.bc_max_steps, profile_events=int(bool(profile_events)),
                     bc_final_only=int(bool(bc_final_only)))
        self.env_kind = self.kind   # the environment the stepenv_* methods step: a KIND_DENSE engine's is the one it was created on
        if self.kind == KIND_DENSE:
            self.hidden = tuple(int(w) for w in (hidden if hasattr(hidden, '__len__') else ((hidden,) if hidden else ())))
            self.nonlin = int(DENSE_NONLINS.get(nonlin, nonlin))
            self.env_kind = int(KIND_MAZE if env is None else env)
            cfg.reserved[0], cfg.reserved[1], cfg.reserved[2] = self.env_kind, len(self.hidden), self.nonlin
            for i, w in enumerate(self.hidden[:3]):
                cfg.reserved[3 + i] = w
            if len(self.hidden) > 3:
                cfg.reserved[1] = len(self.hidden)   # (dne_create refuses it by name)
        else:
            self.hidden = int(hidden)
        if self.kind in MUJOCO_KINDS:
            self.ac_mode, self.nonlin = int(PENDULUM_AC_MODES.get(ac_mode, ac_mode)), int(PENDULUM_NONLINS.get(nonlin, nonlin))
            cfg.reserved[0], cfg.reserved[1], cfg.reserved[2] = self.hidden, self.ac_mode, self.nonlin
        self.bc_final_only = bool(bc_final_only)
        self.h = C.c_void_p()
        rc = self.lib.dne_create(C.byref(cfg), C.byref(self.h))
        if rc != 0:
            raise DneError(self.lib.dne_last_error(None).decode())
        self.P = self.lib.dne_pendulum_num_params(self.hidden, self.n_actions) if self.kind == KIND_PENDULUM else \
            self.lib.dne_mjmaze_num_params(self.hidden, self.n_actions) if self.kind == KIND_MJMAZE else \
            dense_num_params(self.env_kind, self.hidden, self.n_actions) if self.kind == KIND_DENSE else \
            self.lib.dne_num_params(self.kind, self.n_actions)
        self.record_bc = bool(record_bc)
        self.noise_count = 0
        self._last_eval_n = 0   # members of the last es_eval / eval_members (what the maze's xy=None forms score or append by default)
        self.comm_size = 1

    def close(self):
        if getattr(self, "h", None):
            self.lib.dne_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise DneError(self.lib.dne_last_error(self.h).decode())

    # ---- noise / parameters
    def noise_upload(self, noise):
        noise = _arr(noise, np.float32)
        self._ck(self.lib.dne_noise_upload(self.h, _ptr(noise, C.c_float), C.c_size_t(noise.size)))
        self.noise_count = noise.size

    def noise_alloc(self, count):
        self._ck(self.lib.dne_noise_alloc(self.h, C.c_size_t(int(count))))
        self.noise_count = int(count)

    def noise_write(self, offset, chunk):
        chunk = _arr(chunk, np.float32)
        self._ck(self.lib.dne_noise_write(self.h, C.c_size_t(int(offset)), _ptr(chunk, C.c_float), C.c_size_t(chunk.size)))

    def check_redzones(self):
        """0 = no kernel wrote outside its device buffer; raises with the buffer's name otherwise"""
        rc = self.lib.dne_check_redzones(self.h)
        if rc != 0:
            raise DneError(self.lib.dne_last_error(self.h).decode())
        return 0

    def noise_get(self, idx, dim):
        out = np.empty(dim, np.float32)
        self._ck(self.lib.dne_noise_get(self.h, C.c_int64(int(idx)), int(dim), _ptr(out, C.c_float)))
        return out

    def set_theta(self, theta, slot=0):
        theta = _arr(theta, np.float32)
        self._ck(self.lib.dne_set_theta(self.h, int(slot), _ptr(theta, C.c_float), C.c_size_t(theta.size)))

    def get_theta(self, slot=0):
        out = np.empty(self.P, np.float32)
        self._ck(self.lib.dne_get_theta(self.h, int(slot), _ptr(out, C.c_float), C.c_size_t(out.size)))
        return out

    def set_ref_batch(self, ref):
        ref = _arr(ref, np.uint8)
        assert ref.shape[1:] == OB_SHAPE
        self._ck(self.lib.dne_set_ref_batch(self.h, _ptr(ref, C.c_uint8), int(ref.shape[0])))

    def ref_dedup_active(self):
        """(the reference pass runs on the batch's unique operands, U1, U2) -- see dne_ref_dedup_active"""
        u1, u2 = C.c_int(0), C.c_int(0)
        rc = self.lib.dne_ref_dedup_active(self.h, C.byref(u1), C.byref(u2))
        if rc < 0:
            raise DneError(self.lib.dne_last_error(self.h).decode())
        return bool(rc), u1.value, u2.value

    def materialize(self, idx, sigma, copy_out=True):
        idx = _arr(idx, np.int64)
        out = np.empty((idx.size, 2, self.P), np.float32) if copy_out else None
        self._ck(self.lib.dne_materialize(self.h, _ptr(idx, C.c_int64), int(idx.size), C.c_float(sigma), _ptr(out, C.c_float)))
        return out

    # ---- env
    def env_reset(self, seeds):
        seeds = _arr(seeds, np.uint32)
        self._ck(self.lib.dne_env_reset(self.h, int(seeds.size), _ptr(seeds, C.c_uint32)))

    def env_step(self, actions):
        actions = _arr(actions, np.int32)
        n = actions.size
        rew = np.empty(n, np.float32); done = np.empty(n, np.int32)
        self._ck(self.lib.dne_env_step(self.h, n, _ptr(actions, C.c_int32), _ptr(rew, C.c_float), _ptr(done, C.c_int32)))
        return rew, done.astype(bool)

    def env_observation(self, n):
        out = np.empty((n,) + OB_SHAPE, np.uint8)
        self._ck(self.lib.dne_env_observation(self.h, int(n), _ptr(out, C.c_uint8)))
        return out

    def env_ram(self, n):
        out = np.empty((n, RAM_BYTES), np.uint8)
        self._ck(self.lib.dne_env_ram(self.h, int(n), _ptr(out, C.c_uint8)))
        return out

    def env_set_observation(self, obs):
        obs = _arr(obs, np.uint8)
        self._ck(self.lib.dne_env_set_observation(self.h, int(obs.shape[0]), _ptr(obs, C.c_uint8)))

    def env_set_ram(self, ram_prev, ram_cur):
        """inject emulator states (RAM before / after the last raw frame); observations are re-rendered as after a reset"""
        ram_prev = _arr(ram_prev, np.uint8).reshape(-1, RAM_BYTES); ram_cur = _arr(ram_cur, np.uint8).reshape(-1, RAM_BYTES)
        assert ram_prev.shape == ram_cur.shape
        self._ck(self.lib.dne_env_set_ram(self.h, int(ram_prev.shape[0]), _ptr(ram_prev, C.c_uint8), _ptr(ram_cur, C.c_uint8)))

    # ---- forward
    def set_members(self, slot, off, scale):
        slot = _arr(slot, np.int32); off = _arr(off, np.int64); scale = _arr(scale, np.float32)
        assert slot.size == off.size == scale.size
        self._ck(self.lib.dne_set_members(self.h, int(slot.size), _ptr(slot, C.c_int32), _ptr(off, C.c_int64), _ptr(scale, C.c_float)))

    def ref_pass(self, n):
        self._ck(self.lib.dne_ref_pass(self.h, int(n)))

    def get_bn(self, n):
        out = np.empty((n, BN_FLOATS), np.float32)
        self._ck(self.lib.dne_get_bn(self.h, int(n), _ptr(out, C.c_float)))
        return out

    def get_bn_moments(self, n):
        out = np.empty((n, BN_FLOATS), np.float32)
        self._ck(self.lib.dne_get_bn_moments(self.h, int(n), _ptr(out, C.c_float)))
        return out

    def act(self, n):
        actions = np.empty(n, np.int32); logits = np.empty((n, self.n_actions), np.float32)
        self._ck(self.lib.dne_act(self.h, int(n), _ptr(actions, C.c_int32), _ptr(logits, C.c_float)))
        return actions, logits

    def debug_members(self):
        """dne_debug_members: the current members in the engine's order, as the kernels will read them -> (slot int32 [n], off int64 [n],
        scale float32 [n], caller_index int32 [n]); caller_index[j] = the caller's index of engine member j (ga_eval* may reorder)"""
        n = self.lib.dne_debug_members(self.h, 0, None, None, None, None)
        if n < 0:
            raise DneError(self.lib.dne_last_error(self.h).decode())
        slot = np.empty(n, np.int32); off = np.empty(n, np.int64); scale = np.empty(n, np.float32); who = np.empty(n, np.int32)
        got = self.lib.dne_debug_members(self.h, n, _ptr(slot, C.c_int32), _ptr(off, C.c_int64), _ptr(scale, C.c_float), _ptr(who, C.c_int32))
        if got != n:
            raise DneError("dne_debug_members: %d members, then %d" % (n, got))
        return slot, off, scale, who

    def debug_activations_large(self, member):
        """LargeModel: raw conv1 [441*32], conv2 / conv3 [121*64] and fc [512] outputs of one member after act()"""
        y1 = np.empty(14112, np.float32); y2 = np.empty(7744, np.float32); y3 = np.empty(7744, np.float32); y4 = np.empty(512, np.float32)
        self._ck(self.lib.dne_debug_activations_large(self.h, int(member), _ptr(y1, C.c_float), _ptr(y2, C.c_float), _ptr(y3, C.c_float), _ptr(y4, C.c_float)))
        return y1, y2, y3, y4

    def debug_activations(self, member):
        y1 = np.empty(7056, np.float32); y2 = np.empty(3872, np.float32); y3 = np.empty(256, np.float32)
        self._ck(self.lib.dne_debug_activations(self.h, int(member), _ptr(y1, C.c_float), _ptr(y2, C.c_float), _ptr(y3, C.c_float)))
        return y1, y2, y3

    # ---- batch evaluation
    def _bc_buf(self, n, want):
        if not want:
            return None
        if self.kind == KIND_MAZE:   # the navigator's (x, y) after every step
            return np.zeros((n, max(self.bc_max_steps, 1), 2), np.float32)
        if self.kind in ES_KINDS and not self.bc_final_only:
            return np.zeros((n, self.bc_max_steps, RAM_BYTES), np.uint8)
        return np.zeros((n, RAM_BYTES), np.uint8)

    def es_eval(self, noise_idx, sigma, tslimit, env_seed, want_bc=False):
        idx = _arr(noise_idx, np.int64); seeds = _arr(env_seed, np.uint32)
        n = idx.size
        assert seeds.size == 2 * n
        ret = np.empty((n, 2), np.float32); sg = np.empty((n, 2), np.float32); ln = np.empty((n, 2), np.int32)
        bc = self._bc_buf(2 * n, want_bc)
        self._ck(self.lib.dne_es_eval(self.h, _ptr(idx, C.c_int64), n, C.c_float(sigma), int(tslimit), _ptr(seeds, C.c_uint32),
                                      _ptr(ret, C.c_float), _ptr(sg, C.c_float), _ptr(ln, C.c_int32), _ptr(bc, C.c_uint8)))
        self._last_eval_n = 2 * n
        return (ret, sg, ln, bc) if want_bc else (ret, sg, ln)

    def eval_members(self, n, tslimit, env_seed, want_bc=False):
        seeds = _arr(env_seed, np.uint32)
        assert seeds.size == n
        ret = np.empty(n, np.float32); sg = np.empty(n, np.float32); ln = np.empty(n, np.int32)
        bc = self._bc_buf(n, want_bc)
        self._ck(self.lib.dne_eval_members(self.h, int(n), int(tslimit), _ptr(seeds, C.c_uint32), _ptr(ret, C.c_float),
                                           _ptr(sg, C.c_float), _ptr(ln, C.c_int32), _ptr(bc, C.c_uint8)))
        self._last_eval_n = int(n)
        return (ret, sg, ln, bc) if want_bc else (ret, sg, ln)

    def ga_eval(self, chains, sigma, tslimit, env_seed, want_bc=False):
        n = len(chains)
        co = np.zeros(n + 1, np.int32)
        co[1:] = np.cumsum([len(c) for c in chains])
        flat = _arr(np.concatenate([np.asarray(c, np.int64) for c in chains]), np.int64)
        seeds = _arr(env_seed, np.uint32)
        assert seeds.size == n
        ret = np.empty(n, np.float32); sg = np.empty(n, np.float32); ln = np.empty(n, np.int32)
        bc = self._bc_buf(n, want_bc)
        self._ck(self.lib.dne_ga_eval(self.h, _ptr(co, C.c_int32), _ptr(flat, C.c_int64), n, C.c_float(sigma), int(tslimit),
                                      _ptr(seeds, C.c_uint32), _ptr(ret, C.c_float), _ptr(sg, C.c_float), _ptr(ln, C.c_int32),
                                      _ptr(bc, C.c_uint8)))
        self._last_eval_n = n
        return (ret, sg, ln, bc) if want_bc else (ret, sg, ln)

    # ---- the hard maze (KIND_MAZE)
    def maze_set_walls(self, header, lines):
        """the maze every later evaluation runs in: load_maze(path)'s header [8] and lines [n][4], 1 <= n <= 64"""
        header, lines = _maze_args(header, lines)
        self._ck(self.lib.dne_maze_set_walls(self.h, _ptr(header, C.c_float), _ptr(lines, C.c_float), int(lines.shape[0])))

    def maze_final_state(self, n):
        """MazeFinalState: final (x, y) of the first n members of the last evaluation, [n][2]"""
        xy = np.empty((int(n), 2), np.float32)
        self._ck(self.lib.dne_maze_final_state(self.h, int(n), _ptr(xy, C.c_float)))
        return xy

    def maze_debug_trace(self, member, tslimit=MAZE_STEPS):
        """the kernel once more for one current member, every step written out: [min(tslimit, 400)][16] as maze_rollout_host's trace"""
        out = np.empty((min(int(tslimit), MAZE_STEPS), MAZE_TRACE_W), np.float32)
        self._ck(self.lib.dne_maze_debug_trace(self.h, int(member), int(tslimit), _ptr(out, C.c_float)))
        return out

    def maze_debug_math(self, fn, x):
        """maze_math_host's device twin (k_maze_math, one thread per input): [n][2] doubles"""
        x = _arr(x, np.float64).reshape(-1)
        out = np.empty((x.size, 2), np.float64)
        self._ck(self.lib.dne_maze_debug_math(self.h, int(fn), _ptr(x, C.c_double), int(x.size), _ptr(out, C.c_double)))
        return out

    # ---- MujocoPolicy on the pendulum (KIND_PENDULUM) and on the hard maze (KIND_MJMAZE): dne_<name>_* with observations `obs` wide
    def _mujoco_set_ob_stat(self, name, obs, mean, std):
        mean = _arr(mean, np.float32).reshape(obs); std = _arr(std, np.float32).reshape(obs)
        self._ck(getattr(self.lib, "dne_%s_set_ob_stat" % name)(self.h, _ptr(mean, C.c_float), _ptr(std, C.c_float)))

    def _mujoco_set_rollout_options(self, name, n, ac_noise_std, ac_off, stat_flag):
        ac_off = None if ac_off is None else _arr(ac_off, np.int64).reshape(-1)
        stat_flag = None if stat_flag is None else _arr(stat_flag, np.uint8).reshape(-1)
        for a in (ac_off, stat_flag):
            if a is not None and a.size != int(n):
                raise DneError("%s_set_rollout_options: %d members, %d values" % (name, int(n), a.size))
        self._ck(getattr(self.lib, "dne_%s_set_rollout_options" % name)(self.h, int(n), C.c_float(ac_noise_std), _ptr(ac_off, C.c_int64),
                                                                        _ptr(stat_flag, C.c_uint8)))

    def _mujoco_ob_stats(self, name, obs, n):
        s = np.empty((int(n), obs), np.float64); q = np.empty((int(n), obs), np.float64); c = np.empty(int(n), np.int32)
        self._ck(getattr(self.lib, "dne_%s_ob_stats" % name)(self.h, int(n), _ptr(s, C.c_double), _ptr(q, C.c_double), _ptr(c, C.c_int32)))
        return s, q, c

    def _debug_trace(self, name, member, tslimit, cap, width, dtype, init=()):
        """dne_<name>_debug_trace: [steps][width] rows of `dtype`; init: the kind's leading arguments (an initial state or None), if it has any"""
        out = np.zeros((min(int(tslimit), cap), width), dtype)
        steps = C.c_int32(0)
        ct = C.c_double if dtype == np.float64 else C.c_float
        self._ck(getattr(self.lib, "dne_%s_debug_trace" % name)(self.h, int(member), int(tslimit), *init, _ptr(out, ct), C.byref(steps)))
        return out[:steps.value]

    def pendulum_set_ob_stat(self, mean, std):
        self._mujoco_set_ob_stat("pendulum", PENDULUM_OBS, mean, std)

    def pendulum_set_rollout_options(self, n, ac_noise_std=0.0, ac_off=None, stat_flag=None):
        """for the next evaluation only (it must run n members): ac_off int64 [n] -- where each member's 200 action-noise values start in the
        noise table, < 0 for none -- and stat_flag uint8 [n] -- who accumulates the observations it acts on"""
        self._mujoco_set_rollout_options("pendulum", n, ac_noise_std, ac_off, stat_flag)

    def pendulum_ob_stats(self, n):
        """(sum float64 [n][3], sumsq float64 [n][3], count int32 [n]) of the last evaluation's first n members"""
        return self._mujoco_ob_stats("pendulum", PENDULUM_OBS, n)

    def pendulum_final_state(self, n):
        """final (theta, theta_dot) of the last evaluation's first n members, float64 [n][2]"""
        state = np.empty((int(n), 2), np.float64)
        self._ck(self.lib.dne_pendulum_final_state(self.h, int(n), _ptr(state, C.c_double)))
        return state

    def pendulum_debug_trace(self, member, tslimit=PENDULUM_STEPS, init=None):
        """the kernel once more for one current member, every step written out: float64 [steps][8] as pendulum_rollout_host's trace"""
        init = None if init is None else _arr(init, np.float64).reshape(2)
        return self._debug_trace("pendulum", member, tslimit, PENDULUM_STEPS, PENDULUM_TRACE_W, np.float64, (_ptr(init, C.c_double),))

    def pendulum_debug_math(self, fn, x, a=0.0, b=1.0):
        """pendulum_math_host on the device"""
        x = _arr(x, np.float64).reshape(-1)
        out = np.empty(x.size, np.float64)
        self._ck(self.lib.dne_pendulum_debug_math(self.h, int(PENDULUM_MATH.get(fn, fn)), _ptr(x, C.c_double), int(x.size), C.c_float(a), C.c_float(b),
                                                  _ptr(out, C.c_double)))
        return out

    # (KIND_MJMAZE: the walls, the final positions and the archive are the maze_* methods)
    def mjmaze_set_ob_stat(self, mean, std):
        self._mujoco_set_ob_stat("mjmaze", MJMAZE_OBS, mean, std)

    def mjmaze_set_rollout_options(self, n, ac_noise_std=0.0, ac_off=None, stat_flag=None):
        """for the next evaluation only (it must run n members): ac_off int64 [n] -- where each member's 800 action-noise values start in the
        noise table, < 0 for none -- and stat_flag uint8 [n] -- who accumulates the observations it acts on"""
        self._mujoco_set_rollout_options("mjmaze", n, ac_noise_std, ac_off, stat_flag)

    def mjmaze_ob_stats(self, n):
        """(sum float64 [n][11], sumsq float64 [n][11], count int32 [n]) of the last evaluation's first n members"""
        return self._mujoco_ob_stats("mjmaze", MJMAZE_OBS, n)

    def mjmaze_debug_trace(self, member, tslimit=MJMAZE_STEPS):
        """the kernel once more for one current member, every step written out: float32 [steps][20] as mjmaze_rollout_host's trace"""
        return self._debug_trace("mjmaze", member, tslimit, MJMAZE_STEPS, MJMAZE_TRACE_W, np.float32)

    # ---- gym.CartPole-v1 (KIND_CARTPOLE)
    def cartpole_final_state(self, n):
        """final (x, x_dot, theta, theta_dot) of the first n members of the last evaluation, float64 [n][4]"""
        state = np.empty((int(n), 4), np.float64)
        self._ck(self.lib.dne_cartpole_final_state(self.h, int(n), _ptr(state, C.c_double)))
        return state

    def cartpole_debug_trace(self, member, tslimit=CARTPOLE_STEPS, init=None):
        """the kernel once more for one current member, every step written out: float64 [steps][8] as cartpole_rollout_host's trace, cut at the
        episode's length.  init [4]: the initial state; None: the reset of the seed that member had in the last evaluation."""
        init = None if init is None else _arr(init, np.float64).reshape(4)
        return self._debug_trace("cartpole", member, tslimit, CARTPOLE_STEPS, CARTPOLE_TRACE_W, np.float64, (_ptr(init, C.c_double),))

    # ---- the maze, the cart-pole and the pendulum one step at a time (csrc/step_env.h): a batch of max_members environments apart from evaluations
    def _stepenv_idx(self, indices, n=None):
        """(pointer or None, count, the array kept alive): indices=None names environments 0 .. n - 1 (the whole batch without n)"""
        if indices is None:
            return None, int(self.max_members if n is None else n), None
        idx = _arr(indices, np.int32).reshape(-1)
        return _ptr(idx, C.c_int32), int(idx.size), idx

    def stepenv_reset(self, indices=None, seeds=None, max_steps=0, n=None):
        """dne_stepenv_reset: the named environments restart (the maze from its header; the others from seeds uint32 [n]); steps 0, done 0,
        limit = min(max_steps, the kind's own), max_steps <= 0 meaning the own limit"""
        ip, n, _keep = self._stepenv_idx(indices, n)
        if seeds is not None:
            seeds = _arr(seeds, np.uint32).reshape(-1)
            if seeds.size != n:
                raise DneError("stepenv_reset: %d environments, %d seeds" % (n, seeds.size))
        self._ck(self.lib.dne_stepenv_reset(self.h, n, ip, _ptr(seeds, C.c_uint32), int(max_steps)))

    def stepenv_step(self, actions, indices=None, as_int=None):
        """dne_stepenv_step_f32 / _i32 by the dtype the kind takes: one step of the named environments under actions (maze float32 [n][2],
        cart-pole int32 [n], pendulum float32 [n]) -> (reward float32 [n], done bool [n]).  as_int names the entry point outright (the engine
        refuses the one its kind does not take)."""
        is_int = bool(as_int) if as_int is not None else stepenv_dims(self.env_kind)[3] if self.env_kind in STEP_ENVS else np.asarray(actions).dtype.kind in "iu"
        a = _arr(actions, np.int32 if is_int else np.float32)
        ip, n, _keep = self._stepenv_idx(indices, a.shape[0] if a.ndim else 1)
        if as_int is None and self.env_kind in STEP_ENVS and a.size != n * stepenv_dims(self.env_kind)[1]:
            raise DneError("stepenv_step: %d environments take %d action values, %d given" % (n, n * stepenv_dims(self.env_kind)[1], a.size))
        rew = np.empty(n, np.float32); done = np.empty(n, np.uint8)
        if is_int:
            self._ck(self.lib.dne_stepenv_step_i32(self.h, n, ip, _ptr(a, C.c_int32), _ptr(rew, C.c_float), _ptr(done, C.c_uint8)))
        else:
            self._ck(self.lib.dne_stepenv_step_f32(self.h, n, ip, _ptr(a, C.c_float), _ptr(rew, C.c_float), _ptr(done, C.c_uint8)))
        return rew, done.astype(bool)

    def stepenv_observation(self, indices=None, n=None):
        """dne_stepenv_observation: what the policy sees next, float32 [n][OBS] in the order of the list"""
        ip, n, _keep = self._stepenv_idx(indices, n)
        w = stepenv_dims(self.env_kind)[0] if self.env_kind in STEP_ENVS else 1
        out = np.empty((max(n, 0), w), np.float32)
        self._ck(self.lib.dne_stepenv_observation(self.h, n, ip, _ptr(out, C.c_float)))
        return out

    def stepenv_state(self, indices=None, n=None):
        """dne_stepenv_get_state: (state float64 [n][S], steps int32 [n], done bool [n])"""
        ip, n, _keep = self._stepenv_idx(indices, n)
        S = stepenv_dims(self.env_kind)[2] if self.env_kind in STEP_ENVS else 1
        state = np.empty((max(n, 0), S), np.float64); steps = np.empty(max(n, 0), np.int32); done = np.empty(max(n, 0), np.uint8)
        self._ck(self.lib.dne_stepenv_get_state(self.h, n, ip, _ptr(state, C.c_double), _ptr(steps, C.c_int32), _ptr(done, C.c_uint8)))
        return state, steps, done.astype(bool)

    def stepenv_set_state(self, state, steps=None, indices=None, max_steps=0):
        """dne_stepenv_set_state: the named environments are put into states float64 [n][S] with `steps` already taken (default 0); the
        observation is recomputed, done cleared, the limit set as by a reset"""
        S = stepenv_dims(self.env_kind)[2] if self.env_kind in STEP_ENVS else 1
        state = _arr(state, np.float64).reshape(-1, S)
        ip, n, _keep = self._stepenv_idx(indices, state.shape[0])
        steps = np.zeros(n, np.int32) if steps is None else _arr(steps, np.int32).reshape(-1)
        if state.shape[0] != n or steps.size != n:
            raise DneError("stepenv_set_state: %d environments, %d states, %d step counts" % (n, state.shape[0], steps.size))
        self._ck(self.lib.dne_stepenv_set_state(self.h, n, ip, _ptr(state, C.c_double), _ptr(steps, C.c_int32), int(max_steps)))

    def stepenv_last_ms(self):
        """the last step kernel between two device events, milliseconds (-1 before the first)"""
        self.lib.dne_stepenv_last_ms.restype = C.c_double
        return float(self.lib.dne_stepenv_last_ms(self.h))

    # ---- a dense policy behind the environments (KIND_DENSE; csrc/dense.h)
    def _stepenv_members(self, members, n):
        if members is None:
            return None, None
        m = _arr(members, np.int32).reshape(-1)
        if m.size != n:
            raise DneError("stepenv: %d environments, %d members" % (n, m.size))
        return _ptr(m, C.c_int32), m

    def stepenv_act(self, indices=None, members=None, n=None):
        """dne_stepenv_act: the forward pass of member members[i] (None: members[i] = indices[i]) on the current observation of environment
        indices[i] -> (out float32 [n][outputs], actions as stepenv_step takes them)"""
        ip, n, _keep = self._stepenv_idx(indices, n)
        mp, _keep2 = self._stepenv_members(members, n)
        obs_w, act_w, _, is_int = stepenv_dims(self.env_kind) if self.env_kind in STEP_ENVS else (1, 1, 1, False)
        out = np.empty((max(n, 0), self.n_actions), np.float32)
        act = np.empty((max(n, 0), act_w) if act_w > 1 else max(n, 0), np.int32 if is_int else np.float32)
        self._ck(self.lib.dne_stepenv_act(self.h, n, ip, mp, _ptr(out, C.c_float), C.cast(_ptr(act, C.c_int32 if is_int else C.c_float), C.c_void_p)))
        return out, act

    def stepenv_run(self, max_steps, indices=None, members=None, n=None):
        """dne_stepenv_run: max_steps >= 1 rounds of act -> step in one launch from the batch's current state -> (reward_sum float32 [n]: the
        float64 sum of this call's rewards cast once, steps_taken int32 [n], done bool [n])"""
        ip, n, _keep = self._stepenv_idx(indices, n)
        mp, _keep2 = self._stepenv_members(members, n)
        rew = np.empty(max(n, 0), np.float32); steps = np.empty(max(n, 0), np.int32); done = np.empty(max(n, 0), np.uint8)
        self._ck(self.lib.dne_stepenv_run(self.h, n, ip, mp, int(max_steps), _ptr(rew, C.c_float), _ptr(steps, C.c_int32), _ptr(done, C.c_uint8)))
        return rew, steps, done.astype(bool)

    def dense_final_state(self, n):
        """dne_dense_final_state: the final states float64 [n][S] of the last evaluation"""
        S = stepenv_dims(self.env_kind)[2] if self.env_kind in STEP_ENVS else 1
        out = np.empty((max(int(n), 0), S), np.float64)
        self._ck(self.lib.dne_dense_final_state(self.h, int(n), _ptr(out, C.c_double)))
        return out

    # ---- novelty over final states on a dense policy (csrc/dense_novelty.h): BCs are D floats of the final state, the archive lives on the device
    def dense_bc_dim(self):
        D = self.lib.dne_dense_bc_dim(self.h)
        if D < 0:
            self._ck(D)
        return D

    def dense_bc(self, n):
        """dne_dense_bc: the BCs float32 [n][D] of the last evaluation's first n members"""
        out = np.empty((max(int(n), 0), self.dense_bc_dim()), np.float32)
        self._ck(self.lib.dne_dense_bc(self.h, int(n), _ptr(out, C.c_float)))
        return out

    # ---- the device-resident archive and its novelty, once for the maze_* and dense_* methods below: `family` is the C prefix ('maze': points of
    # width 2, csrc/maze_novelty.h; 'dense': BCs of width dense_bc_dim(), csrc/dense_novelty.h), and the entry point is dne_<family>_<name>
    def _width(self, family):
        return 2 if family == 'maze' else self.dense_bc_dim()

    def _points(self, family, points, n):
        """(host points or None, count): points=None means the first n members of the last evaluation (all of them without n), read on the device"""
        if points is None:
            return None, int(self._last_eval_n if n is None else n)
        points = _arr(points, np.float32).reshape(-1, self._width(family))
        if n is not None and int(n) != points.shape[0]:
            raise DneError("%d points given, n = %d" % (points.shape[0], int(n)))
        return points, int(points.shape[0])

    def _archive_append(self, family, points, n):
        points, n = self._points(family, points, n)
        self._ck(getattr(self.lib, 'dne_%s_archive_append' % family)(self.h, _ptr(points, C.c_float), n))

    def _archive_size(self, family):
        n = getattr(self.lib, 'dne_%s_archive_size' % family)(self.h)
        if n < 0:
            self._ck(n)
        return n

    def _archive(self, family):
        n = self._archive_size(family)
        out = np.empty((n, self._width(family)), np.float32)
        self._ck(getattr(self.lib, 'dne_%s_archive_get' % family)(self.h, _ptr(out, C.c_float), n))
        return out

    def _novelty(self, family, name, k, points, n):
        """name 'novelty' or 'novelty_pool' -> float64 [n]"""
        points, n = self._points(family, points, n)
        out = np.empty(max(n, 0), np.float64)
        self._ck(getattr(self.lib, 'dne_%s_%s' % (family, name))(self.h, _ptr(points, C.c_float), n, int(k), _ptr(out, C.c_double)))
        return out

    def _archive_append_members(self, family, members):
        members = _arr(members, np.int32).reshape(-1)
        self._ck(getattr(self.lib, 'dne_%s_archive_append_members' % family)(self.h, _ptr(members, C.c_int32), int(members.size)))

    def _novelty_last_ms(self, family):
        fn = getattr(self.lib, 'dne_%s_novelty_last_ms' % family)
        fn.restype = C.c_double
        return float(fn(self.h))

    def dense_archive_append(self, bc=None, n=None):
        """append BCs [n][D] to the device-resident archive, in order; bc=None: those of the last evaluation's first n members, device to device"""
        self._archive_append('dense', bc, n)

    def dense_archive_clear(self):
        self._ck(self.lib.dne_dense_archive_clear(self.h))

    def dense_archive_size(self):
        return self._archive_size('dense')

    def dense_archive(self):
        """the archive's BCs in insertion order, [size][D] float32"""
        return self._archive('dense')

    def dense_novelty(self, k, bc=None, n=None):
        """nses.py:22-32 on BCs of D floats: the mean distance of each to its min(k, archive size) nearest archive points, float64 [n]
        (k_dense_novelty; 1 <= k <= DENSE_NOVELTY_KMAX).  bc=None scores the last evaluation's first n members on the device."""
        return self._novelty('dense', 'novelty', k, bc, n)

    def dense_novelty_pool(self, k, bc=None, n=None):
        """GA-NS's novelty on BCs of D floats: the mean distance of each to its min(k, archive size + n - 1) nearest among the archive's points
        and the OTHER n - 1 BCs, float64 [n] (k_dense_novelty_pool; 1 <= k <= DENSE_NOVELTY_KMAX).  bc=None scores the last evaluation's first
        n members on the device."""
        return self._novelty('dense', 'novelty_pool', k, bc, n)

    def dense_archive_append_members(self, members):
        """append the BCs of the last evaluation's members `members` (indices, in this order, repeats allowed) to the archive, device to device"""
        self._archive_append_members('dense', members)

    def dense_novelty_last_ms(self):
        """the scoring kernel of the last dense_novelty / dense_novelty_pool call between two device events, milliseconds (-1 before the first)"""
        return self._novelty_last_ms('dense')

    # ---- novelty on the hard maze (csrc/maze_novelty.h): BCs are final (x, y) points, the archive lives on the device
    def maze_archive_append(self, xy=None, n=None):
        """append points [n][2] to the device-resident archive, in order; xy=None: the final positions of the last evaluation's first n
        members, device to device"""
        self._archive_append('maze', xy, n)

    def maze_archive_clear(self):
        self._ck(self.lib.dne_maze_archive_clear(self.h))

    def maze_archive_size(self):
        return self._archive_size('maze')

    def maze_archive(self):
        """the archive's points in insertion order, [size][2] float32"""
        return self._archive('maze')

    def maze_novelty(self, k, xy=None, n=None):
        """nses.py:22-32 on (x, y) points: the mean distance of each point to its min(k, archive size) nearest archive points, float64 [n]
        (k_maze_novelty; 1 <= k <= MAZE_NOVELTY_KMAX).  xy=None scores the last evaluation's first n members where the rollout left them."""
        return self._novelty('maze', 'novelty', k, xy, n)

    def maze_novelty_pool(self, k, xy=None, n=None):
        """GA-NS's novelty: the mean distance of each point to its min(k, archive size + n - 1) nearest among the archive's points and the
        OTHER n - 1 points, float64 [n] (k_maze_novelty_pool; 1 <= k <= MAZE_NOVELTY_KMAX).  xy=None scores the last evaluation's first n
        members where the rollout left them."""
        return self._novelty('maze', 'novelty_pool', k, xy, n)

    def maze_archive_append_members(self, members):
        """append the final positions of the last evaluation's members `members` (indices, in this order, repeats allowed) to the archive,
        device to device"""
        self._archive_append_members('maze', members)

    def maze_novelty_last_ms(self):
        """the scoring kernel of the last maze_novelty / maze_novelty_pool call between two device events, milliseconds"""
        return self._novelty_last_ms('maze')

    # ---- Deep-GA on the hard maze (csrc/maze_ga.h): the parents live in a bank on the device, a member is (parent, idx, power)
    def maze_ga_set_init_scale(self, scale_by):
        sb = _arr(scale_by, np.float32)
        self._ck(self.lib.dne_maze_ga_set_init_scale(self.h, _ptr(sb, C.c_float), C.c_size_t(sb.size)))

    @staticmethod
    def _pack_genomes(genomes):
        """(T, chain_offsets int32 [T + 1], indices int64, powers float32) of genomes (idx0, (idx1, power1), ...)"""
        T = len(genomes)
        co = np.zeros(T + 1, np.int32)
        parts = [split_genome(g) for g in genomes]
        co[1:] = np.cumsum([p[0].size for p in parts])
        flat = _arr(np.concatenate([p[0] for p in parts]) if parts else np.zeros(0), np.int64)
        pw = _arr(np.concatenate([p[1] for p in parts]) if parts else np.zeros(0), np.float32)
        return T, co, flat, pw

    def maze_ga_build(self, genomes):
        """the bank = these genomes' thetas, parent j from genomes[j] = (idx0, (idx1, power1), ...)"""
        T, co, flat, pw = self._pack_genomes(genomes)
        self._ck(self.lib.dne_maze_ga_build(self.h, T, _ptr(co, C.c_int32), _ptr(flat, C.c_int64), _ptr(pw, C.c_float)))

    def maze_ga_eval(self, parent, idx, power, tslimit=MAZE_STEPS):
        """one episode per member (parent -1: a root at idx; otherwise bank[parent] + fl(power * noise[idx])) -> (returns, signs, lengths)"""
        parent, idx, power = _maze_ga_members(parent, idx, power)
        n = parent.size
        ret = np.empty(n, np.float32); sg = np.empty(n, np.float32); ln = np.empty(n, np.int32)
        self._ck(self.lib.dne_maze_ga_eval(self.h, n, _ptr(parent, C.c_int32), _ptr(idx, C.c_int64), _ptr(power, C.c_float), int(tslimit),
                                           _ptr(ret, C.c_float), _ptr(sg, C.c_float), _ptr(ln, C.c_int32)))
        self._last_eval_n = n
        return ret, sg, ln

    def maze_ga_promote(self, parent, idx, power):
        """new parent j = the theta of descriptor j over the bank as it is (idx < 0: parent[j] itself), all at once"""
        parent, idx, power = _maze_ga_members(parent, idx, power)
        self._ck(self.lib.dne_maze_ga_promote(self.h, int(parent.size), _ptr(parent, C.c_int32), _ptr(idx, C.c_int64), _ptr(power, C.c_float)))

    def maze_ga_parents(self):
        n = self.lib.dne_maze_ga_parents(self.h)
        if n < 0:
            self._ck(n)
        return n

    def maze_ga_get_parent(self, j):
        out = np.empty(self.P, np.float32)
        self._ck(self.lib.dne_maze_ga_get_parent(self.h, int(j), _ptr(out, C.c_float)))
        return out

    # ---- Deep-GA on a dense policy (csrc/dense_ga.h): the same surface on a KIND_DENSE engine of any shape, P the engine's
    def dense_ga_set_init_scale(self, scale_by):
        sb = _arr(scale_by, np.float32)
        self._ck(self.lib.dne_dense_ga_set_init_scale(self.h, _ptr(sb, C.c_float), C.c_size_t(sb.size)))

    def dense_ga_build(self, genomes):
        """the bank = these genomes' thetas, parent j from genomes[j] = (idx0, (idx1, power1), ...)"""
        T, co, flat, pw = self._pack_genomes(genomes)
        self._ck(self.lib.dne_dense_ga_build(self.h, T, _ptr(co, C.c_int32), _ptr(flat, C.c_int64), _ptr(pw, C.c_float)))

    def dense_ga_eval(self, parent, idx, power, tslimit, env_seed=None):
        """one episode per member (parent -1: a root at idx; otherwise bank[parent] + fl(power * noise[idx])), member i reset from env_seed[i]
        (the cart-pole and the pendulum need it; the maze reads none) -> (returns, signs, lengths)"""
        parent, idx, power = _maze_ga_members(parent, idx, power)
        n = parent.size
        seeds = None if env_seed is None else _arr(env_seed, np.uint32).reshape(-1)
        if seeds is not None and seeds.size != n:
            raise DneError("dense_ga_eval: %d members, %d environment seeds" % (n, seeds.size))
        ret = np.empty(n, np.float32); sg = np.empty(n, np.float32); ln = np.empty(n, np.int32)
        self._ck(self.lib.dne_dense_ga_eval(self.h, n, _ptr(parent, C.c_int32), _ptr(idx, C.c_int64), _ptr(power, C.c_float), _ptr(seeds, C.c_uint32),
                                            int(tslimit), _ptr(ret, C.c_float), _ptr(sg, C.c_float), _ptr(ln, C.c_int32)))
        self._last_eval_n = n
        return ret, sg, ln

    def dense_ga_promote(self, parent, idx, power):
        """new parent j = the theta of descriptor j over the bank as it is (idx < 0: parent[j] itself), all at once"""
        parent, idx, power = _maze_ga_members(parent, idx, power)
        self._ck(self.lib.dne_dense_ga_promote(self.h, int(parent.size), _ptr(parent, C.c_int32), _ptr(idx, C.c_int64), _ptr(power, C.c_float)))

    def dense_ga_parents(self):
        n = self.lib.dne_dense_ga_parents(self.h)
        if n < 0:
            self._ck(n)
        return n

    def dense_ga_get_parent(self, j):
        out = np.empty(self.P, np.float32)
        self._ck(self.lib.dne_dense_ga_get_parent(self.h, int(j), _ptr(out, C.c_float)))
        return out

    # ---- Deep-GA on MujocoPolicy (csrc/mujoco_ga.h): the same surface on a KIND_PENDULUM or KIND_MJMAZE engine; a root is the policy
    # reinitialised on its noise slice, so there is no init scale to set -- the bank is reserved for T_max parents instead
    def mujoco_ga_reserve(self, T_max):
        self._ck(self.lib.dne_mujoco_ga_reserve(self.h, int(T_max)))

    def mujoco_ga_build(self, genomes):
        """the bank = these genomes' thetas, parent j from genomes[j] = (idx0, (idx1, power1), ...)"""
        T, co, flat, pw = self._pack_genomes(genomes)
        self._ck(self.lib.dne_mujoco_ga_build(self.h, T, _ptr(co, C.c_int32), _ptr(flat, C.c_int64), _ptr(pw, C.c_float)))

    def mujoco_ga_eval(self, parent, idx, power, tslimit, env_seed=None):
        """one episode per member (parent -1: a root at idx; otherwise bank[parent] + fl(power * noise[idx])), member i reset from env_seed[i]
        (the pendulum needs it; the maze reads none) -> (returns, signs, lengths).  set_rollout_options applies, ob_stats / final_state follow"""
        parent, idx, power = _maze_ga_members(parent, idx, power)
        n = parent.size
        seeds = None if env_seed is None else _arr(env_seed, np.uint32).reshape(-1)
        if seeds is not None and seeds.size != n:
            raise DneError("mujoco_ga_eval: %d members, %d environment seeds" % (n, seeds.size))
        ret = np.empty(n, np.float32); sg = np.empty(n, np.float32); ln = np.empty(n, np.int32)
        self._ck(self.lib.dne_mujoco_ga_eval(self.h, n, _ptr(parent, C.c_int32), _ptr(idx, C.c_int64), _ptr(power, C.c_float), _ptr(seeds, C.c_uint32),
                                             int(tslimit), _ptr(ret, C.c_float), _ptr(sg, C.c_float), _ptr(ln, C.c_int32)))
        self._last_eval_n = n
        return ret, sg, ln

    def mujoco_ga_promote(self, parent, idx, power):
        """new parent j = the theta of descriptor j over the bank as it is (idx < 0: parent[j] itself), all at once"""
        parent, idx, power = _maze_ga_members(parent, idx, power)
        self._ck(self.lib.dne_mujoco_ga_promote(self.h, int(parent.size), _ptr(parent, C.c_int32), _ptr(idx, C.c_int64), _ptr(power, C.c_float)))

    def mujoco_ga_parents(self):
        n = self.lib.dne_mujoco_ga_parents(self.h)
        if n < 0:
            self._ck(n)
        return n

    def mujoco_ga_get_parent(self, j):
        out = np.empty(self.P, np.float32)
        self._ck(self.lib.dne_mujoco_ga_get_parent(self.h, int(j), _ptr(out, C.c_float)))
        return out

    # ---- gpu-tree genomes: ((idx0,), (idx1, power1), ...)
    def ga_set_init_scale(self, scale_by):
        sb = _arr(scale_by, np.float32)
        self._ck(self.lib.dne_ga_set_init_scale(self.h, _ptr(sb, C.c_float), C.c_size_t(sb.size)))

    @staticmethod
    def _split_powers(chain):
        idx = np.array([c[0] if isinstance(c, (tuple, list)) else c for c in chain], np.int64)
        pw = np.array([c[1] if isinstance(c, (tuple, list)) and len(c) > 1 else 0.0 for c in chain], np.float32)
        return idx, pw

    def ga_rebuild_powers(self, slot, seeds, copy_out=True):
        idx, pw = self._split_powers(seeds)
        out = np.empty(self.P, np.float32) if copy_out else None
        self._ck(self.lib.dne_ga_rebuild_powers(self.h, int(slot), _ptr(idx, C.c_int64), _ptr(pw, C.c_float), int(idx.size), _ptr(out, C.c_float)))
        return out

    def ga_eval_powers(self, genomes, tslimit, env_seed, want_bc=False):
        n = len(genomes)
        co = np.zeros(n + 1, np.int32)
        co[1:] = np.cumsum([len(g) for g in genomes])
        parts = [self._split_powers(g) for g in genomes]
        flat = _arr(np.concatenate([p[0] for p in parts]), np.int64)
        pw = _arr(np.concatenate([p[1] for p in parts]), np.float32)
        seeds = _arr(env_seed, np.uint32)
        assert seeds.size == n
        ret = np.empty(n, np.float32); sg = np.empty(n, np.float32); ln = np.empty(n, np.int32)
        bc = self._bc_buf(n, want_bc)
        self._ck(self.lib.dne_ga_eval_powers(self.h, _ptr(co, C.c_int32), _ptr(flat, C.c_int64), _ptr(pw, C.c_float), n, int(tslimit),
                                             _ptr(seeds, C.c_uint32), _ptr(ret, C.c_float), _ptr(sg, C.c_float), _ptr(ln, C.c_int32),
                                             _ptr(bc, C.c_uint8)))
        self._last_eval_n = n
        return (ret, sg, ln, bc) if want_bc else (ret, sg, ln)

    def ga_rebuild(self, slot, seeds, sigma, copy_out=True):
        seeds = _arr(seeds, np.int64)
        out = np.empty(self.P, np.float32) if copy_out else None
        self._ck(self.lib.dne_ga_rebuild(self.h, int(slot), _ptr(seeds, C.c_int64), int(seeds.size), C.c_float(sigma), _ptr(out, C.c_float)))
        return out

    # ---- reduce
    def centered_ranks(self, x):
        x = _arr(x, np.float32)
        out = np.empty(x.size, np.float32)
        self._ck(self.lib.dne_centered_ranks(self.h, _ptr(x.reshape(-1), C.c_float), int(x.size), _ptr(out, C.c_float)))
        return out.reshape(x.shape)

    def weighted_sum(self, idx, w, denom, copy_out=True):
        idx = _arr(idx, np.int64); w = _arr(w, np.float32)
        g = np.empty(self.P, np.float32) if copy_out else None
        self._ck(self.lib.dne_weighted_sum(self.h, _ptr(idx, C.c_int64), _ptr(w, C.c_float), int(idx.size), C.c_float(denom), _ptr(g, C.c_float)))
        return g

    def optimizer_reset(self):
        self._ck(self.lib.dne_optimizer_reset(self.h))

    def optimizer_get_state(self):
        m = np.empty(self.P, np.float32); v = np.empty(self.P, np.float32); t = C.c_int32()
        self._ck(self.lib.dne_optimizer_get_state(self.h, _ptr(m, C.c_float), _ptr(v, C.c_float), C.byref(t)))
        return m, v, t.value

    def optimizer_set_state(self, m, v, t):
        m = _arr(m, np.float32); v = _arr(v, np.float32)
        self._ck(self.lib.dne_optimizer_set_state(self.h, _ptr(m, C.c_float), _ptr(v, C.c_float), int(t)))

    def optimizer_step(self, kind, l2coeff, stepsize, beta1_or_momentum=0.9, beta2=0.999, epsilon=1e-8):
        ratio = C.c_double()
        self._ck(self.lib.dne_optimizer_step(self.h, OPT_KINDS[kind], C.c_float(l2coeff), C.c_double(stepsize),
                                             C.c_double(beta1_or_momentum), C.c_double(beta2), C.c_double(epsilon), C.byref(ratio)))
        return ratio.value

    def es_update(self, idx, returns_n2, signreturns_n2, proc_mode, opt_kind, l2coeff, stepsize,
                  beta1_or_momentum=0.9, beta2=0.999, epsilon=1e-8):
        idx = _arr(idx, np.int64); r = _arr(returns_n2, np.float32)
        s = _arr(signreturns_n2, np.float32) if signreturns_n2 is not None else None
        ratio = C.c_double()
        self._ck(self.lib.dne_es_update(self.h, _ptr(idx, C.c_int64), _ptr(r, C.c_float), _ptr(s, C.c_float), int(idx.size),
                                        PROC_MODES[proc_mode], OPT_KINDS[opt_kind], C.c_float(l2coeff), C.c_double(stepsize),
                                        C.c_double(beta1_or_momentum), C.c_double(beta2), C.c_double(epsilon), C.byref(ratio)))
        return ratio.value

    # ---- exchange between GPUs (RCCL behind the C ABI; the host transports use pack / set)
    def comm_init(self, rank, nranks, unique_id):
        assert len(unique_id) == 128
        buf = (C.c_char * 128).from_buffer_copy(unique_id)
        rc = self.lib.dne_comm_init(self.h, int(rank), int(nranks), buf)
        if rc == -2:   # DNE_COMM_DROPPED: the late path must not touch the handle's error text (another thread owns the handle by now)
            raise DneError("dne_comm_init: communicator dropped, dne_comm_abort was called while ncclCommInitRank was in flight")
        self._ck(rc)
        self.comm_size = int(nranks)

    def comm_share(self, owner):
        """take part in the RCCL communicator another engine of this process (same device) built with comm_init"""
        self._ck(self.lib.dne_comm_share(self.h, owner.h))
        self.comm_size = owner.comm_size

    def comm_abort(self):
        self._ck(self.lib.dne_comm_abort(self.h))
        self.comm_size = 1

    def comm_info(self):
        """(rank, nranks, is_rccl) as the communicator itself reports them (ncclCommUserRank / ncclCommCount)"""
        r, n, k = C.c_int(), C.c_int(), C.c_int()
        self._ck(self.lib.dne_comm_info(self.h, C.byref(r), C.byref(n), C.byref(k)))
        return r.value, n.value, bool(k.value)

    def comm_allreduce(self, values, op="sum"):
        v = np.array(values, np.float64).reshape(-1)
        self._ck(self.lib.dne_comm_allreduce(self.h, _ptr(v, C.c_double), int(v.size), {"sum": 0, "max": 1}[op]))
        return v

    def barrier(self):
        self._ck(self.lib.dne_comm_allreduce(self.h, None, 0, 0))

    def comm_allgather(self, arr):
        """every rank's `arr` (same shape and dtype everywhere) stacked in rank order"""
        arr = np.ascontiguousarray(arr)
        world = self.comm_size
        out = np.empty((world,) + arr.shape, arr.dtype)
        self._ck(self.lib.dne_comm_allgather(self.h, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes),
                                             out.ctypes.data_as(C.c_void_p)))
        return out

    def allgather_results(self, n_local, n_global):
        rec = np.zeros(int(n_global), RECORD)
        self._ck(self.lib.dne_allgather_results(self.h, int(n_local), int(n_global), rec.ctypes.data_as(C.c_void_p)))
        return rec

    def debug_unshard(self, gathered, n_global, world):
        g = np.ascontiguousarray(gathered, RECORD)
        out = np.zeros(int(n_global), RECORD)
        self._ck(self.lib.dne_debug_unshard(self.h, g.ctypes.data_as(C.c_void_p), int(n_global), int(world), out.ctypes.data_as(C.c_void_p)))
        return out

    def records_pack(self, n_local):
        rec = np.zeros(int(n_local), RECORD)
        self._ck(self.lib.dne_records_pack(self.h, int(n_local), rec.ctypes.data_as(C.c_void_p)))
        return rec

    def records_set(self, rec):
        rec = np.ascontiguousarray(rec, RECORD)
        self._ck(self.lib.dne_records_set(self.h, rec.ctypes.data_as(C.c_void_p), int(rec.size)))

    def es_update_gathered(self, proc_mode, opt_kind, l2coeff, stepsize, beta1_or_momentum=0.9, beta2=0.999, epsilon=1e-8):
        ratio = C.c_double()
        self._ck(self.lib.dne_es_update_gathered(self.h, PROC_MODES[proc_mode], OPT_KINDS[opt_kind], C.c_float(l2coeff),
                                                 C.c_double(stepsize), C.c_double(beta1_or_momentum), C.c_double(beta2),
                                                 C.c_double(epsilon), C.byref(ratio)))
        return ratio.value

    def ga_select(self, returns, t):
        r = _arr(returns, np.float32)
        out = np.empty(t, np.int32)
        self._ck(self.lib.dne_ga_select(self.h, _ptr(r, C.c_float), int(r.size), int(t), _ptr(out, C.c_int32)))
        return out

    def _sync_archive(self, archive):
        """Bring the device-resident archive up to `archive`.  The master's archive only grows (dist.py:93-98) and the
        transport hands back the same entry objects on every call, so entries are recognised by identity and only new ones
        are uploaded; any other list (fresh arrays, a shorter archive) is uploaded from scratch."""
        if archive is None:                  # the resident archive as it stands (what archive_append_members / archive_append_points built)
            return
        have = getattr(self, "_arch_objs", [])
        if len(have) > len(archive) or any(a is not b for a, b in zip(have, archive)):
            self._ck(self.lib.dne_archive_clear(self.h))
            have = []
        for a in archive[len(have):]:
            u = _arr(a, np.uint8)
            u = u.reshape(-1, u.shape[-1])
            self._ck(self.lib.dne_archive_append(self.h, _ptr(u, C.c_uint8), int(u.shape[0]), int(u.shape[1])))
        self._arch_objs = list(archive)      # references keep the identities from being recycled

    # ---- pool novelty over final RAM states (GA-NS on Atari; csrc/ram_novelty.h)
    def ram_novelty_pool(self, k, bc=None, n=None, neighbours=False):
        """dne_ram_novelty_pool: the mean distance of each of n RAM points to its kk = min(k, A + n - 1) nearest among the resident archive's A
        points and the OTHER n - 1 points, float64 [n] (k_ram_novelty_pool; 1 <= k <= RAM_NOVELTY_KMAX).  bc=None scores the last evaluation's
        first n members (all of them by default) where the evaluation left their final RAM, in the caller's member order; bc uint8 [n][128]
        scores host points.  With neighbours also int32 [n][kk]: each member's nearest combined slots, in order."""
        if bc is not None:
            bc = _arr(bc, np.uint8).reshape(-1, RAM_BYTES)
            n = int(bc.shape[0])
        elif n is None:
            n = self._last_eval_n
        n = int(n)
        out = np.empty(max(n, 0), np.float64)
        kk = max(min(int(k), self.archive_size() + n - 1), 0)
        nb = np.empty((max(n, 0), kk), np.int32) if neighbours else None
        self._ck(self.lib.dne_ram_novelty_pool(self.h, _ptr(bc, C.c_uint8), n, int(k), _ptr(out, C.c_double), _ptr(nb, C.c_int32)))
        return (out, nb) if neighbours else out

    def archive_append_members(self, members):
        """dne_archive_append_members: the final RAM of the last evaluation's members `members` (the caller's indices, in that order, repeats
        allowed) become archive entries of length 1, device to device"""
        members = _arr(np.asarray(members).reshape(-1), np.int32)
        self._ck(self.lib.dne_archive_append_members(self.h, _ptr(members, C.c_int32), int(members.size)))
        self._arch_objs = list(getattr(self, "_arch_objs", [])) + [object() for _ in range(members.size)]   # entries no host list holds

    def archive_get_points(self, first, count):
        """dne_archive_get_points: entries first .. first + count - 1 of the resident archive, each of length 1, as uint8 [count][128]"""
        out = np.empty((max(int(count), 0), RAM_BYTES), np.uint8)
        self._ck(self.lib.dne_archive_get_points(self.h, int(first), int(count), _ptr(out, C.c_uint8)))
        return out

    def archive_size(self):
        return int(self.lib.dne_archive_size(self.h))

    def archive_clear(self):
        self._ck(self.lib.dne_archive_clear(self.h))
        self._arch_objs = []

    def archive_append_points(self, points):
        """each row of points uint8 [m][128] becomes an archive entry of length 1 (dne_archive_append, one call per row)"""
        points = _arr(points, np.uint8).reshape(-1, RAM_BYTES)
        for row in points:
            self._ck(self.lib.dne_archive_append(self.h, _ptr(row, C.c_uint8), 1, RAM_BYTES))
        self._arch_objs = list(getattr(self, "_arch_objs", [])) + [object() for _ in range(len(points))]

    def ram_novelty_last_ms(self):
        """the scoring kernel of the last ram_novelty_pool call between two device events, milliseconds (-1 before the first)"""
        self.lib.dne_ram_novelty_last_ms.restype = C.c_double
        return float(self.lib.dne_ram_novelty_last_ms(self.h))

    def novelty(self, archive, bc, k):
        bc = _arr(bc, np.uint8).reshape(-1, np.asarray(bc).shape[-1])
        self._sync_archive(archive)
        out = C.c_double()
        self._ck(self.lib.dne_novelty(self.h, None, None, 0, _ptr(bc, C.c_uint8), int(bc.shape[0]), int(bc.shape[1]), int(k),
                                      C.byref(out)))
        return out.value

    def novelty_batch(self, archive, lengths, k):
        """novelty of every member's RAM trajectory recorded by the last es_eval (kept on the device)"""
        self._sync_archive(archive)
        ln = _arr(np.asarray(lengths).reshape(-1), np.int32)
        out = np.empty(ln.size, np.float64)
        self._ck(self.lib.dne_novelty_batch(self.h, None, None, 0, int(ln.size), _ptr(ln, C.c_int32), int(k), _ptr(out, C.c_double)))
        return out

    def novelty_knn(self, archive, k, bcs=None, lengths=None):
        """novelty of a batch on the device (dne_novelty_knn): `bcs` a list of u8[T][dim] host trajectories (lengths from
        their shapes), or None for the trajectories recorded by the last es_eval / eval_members, `lengths` rows each"""
        self._sync_archive(archive)
        if bcs is None:
            if lengths is None:
                raise DneError("novelty_knn: the recorded trajectories need their lengths")
            ln = _arr(np.asarray(lengths).reshape(-1), np.int32)
            rows, dim = None, RAM_BYTES
        else:
            rs = [_arr(b, np.uint8) for b in bcs]
            rs = [r.reshape(-1, r.shape[-1]) for r in rs]
            if not rs or len({r.shape[1] for r in rs}) != 1:
                raise DneError("novelty_knn: bcs must be a non-empty list of trajectories of one width")
            ln = np.array([r.shape[0] for r in rs], np.int32)
            rows, dim = np.ascontiguousarray(np.concatenate(rs, axis=0)), rs[0].shape[1]
        out = np.empty(ln.size, np.float64)
        self._ck(self.lib.dne_novelty_knn(self.h, _ptr(rows, C.c_uint8), _ptr(ln, C.c_int32), int(ln.size), int(dim), int(k),
                                          _ptr(out, C.c_double)))
        return out

    def profile(self):
        p = Profile()
        self._ck(self.lib.dne_get_profile(self.h, C.byref(p)))
        return {f[0]: getattr(p, f[0]) for f in Profile._fields_ if f[0] != "reserved"}
