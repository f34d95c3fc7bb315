"""TEST-ONLY support for the hard maze (DNE_KIND_MAZE, csrc/maze.h): the fixtures, the tolerances of the comparison with the reference's
two recordings, the edge mazes, the math probe's inputs and measured bounds, a NaN-aware bit comparison, synthetic mazes, member sets, a float32 numpy statement of the policy, and MazeHostEngine -- dne_maze_rollout_host (the same
header compiled for the CPU) behind the Engine method surface, as tests/oracle_engine.py puts the oracle behind it."""
import os

import numpy as np

from oracle_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAZE_FILE = os.path.join(ROOT, "tests", "golden", "hard_maze.txt")
RECORDING = os.path.join(ROOT, "tests", "golden", "maze_reference_rollouts.npz")
P, OBS, STEPS = 498, 11, 400
W1, B1, W2, B2, W3, B3 = 0, 176, 192, 448, 464, 496

# ---- the host restatement against the reference's recording (tests/golden/make_maze_golden.py: g++ -O2, glibc 2.35) -----------------------
# Measured between dne_maze_actions_host and the recording over its 32 sequences x 400 steps:
#   x, y, heading, speed, ang_vel, reward        every one of the 12800 rows bit-identical          (largest difference 0)
#   collision counts, radar bits, reward's step  identical (they are compared exactly in any case)
#   rangefinder observations (range / 100)       152 of 12800 rows differ, largest difference 7.152557373046875e-07 (sequence 2)
# which is what the issue measured on the reference alone when its float trig is replaced by a correctly rounded one (positions bit-identical,
# 98.6 % of rows identical, 4.8e-7): this header's float sine, cosine and arctangent are evaluated in double and rounded once.
# Each bound is four times the measured value (the margin covers libm builds whose float trig differs in the last place):
MEASURED_RANGEFINDER = 7.152557373046875e-07
TOL_RANGEFINDER = 4 * MEASURED_RANGEFINDER          # 2.86e-06
TOL_STATE = 4 * 0.0                                 # x, y, heading, speed, ang_vel, reward: exact
# No wall comparison flipped (every collision count and every rangefinder hit agrees on every step), so no sequence is set aside:
SET_ASIDE = {}                                      # sequence -> step index of the flipped comparison; at most one entry is allowed


# ---- the edge recording (tests/golden/maze_reference_edges.npz: six edge mazes x eleven sequences, NaN / inf / 1e30 / denormal actions included) --
# Measured between dne_maze_actions_host and that recording over its 66 sequences x 400 steps:
#   x, y, heading, speed, ang_vel, reward        NaN where the reference has NaN, bit-identical elsewhere (-0.0 == 0.0 for the reward)
#   collision counts, radar bits, reward's step  identical
#   rangefinder observations (range / 100)       largest difference MEASURED_RANGEFINDER_EDGES
# which is below MEASURED_RANGEFINDER, so the edge recording is held to the same TOL_RANGEFINDER.
EDGE_RECORDING = os.path.join(ROOT, "tests", "golden", "maze_reference_edges.npz")
EDGE_MAZES = ("disable", "zero_wall", "dist_8", "dist_7_99", "goal_on_start", "ray_endpoint")
EDGE_SEQS = ("still", "straight", "spin", "mixed", "wait_then_straight", "nan_turn_from_10", "nan_speed_from_50", "inf_inf", "ninf_1e30",
             "n1e30_ninf", "denormal")
MEASURED_RANGEFINDER_EDGES = 2.384185791015625e-07
SET_ASIDE_EDGES = {}                                # (maze, sequence) -> step index of a flipped wall comparison; at most one entry is allowed


def edge_maze_file(name):
    return os.path.join(ROOT, "tests", "golden", "maze_edge_%s.txt" % name)


def edge_maze(name):
    from dne_hip import _lib
    return _lib.load_maze(edge_maze_file(name))


def same_nan(a, b):
    """equal shapes, NaN exactly where the other has NaN (payload and sign of a NaN are free), equal bits everywhere else"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


# ---- the math probe (dne_maze_math_host / dne_maze_debug_math: sincos_d, atan_d and their float forms outside an episode) ---------------------
# Measured on math_inputs(fn) against the high-precision reference (tests/test_maze_cpu.py says how it is formed):
#   sincos_d, atan_d          largest ABSOLUTE error of the double result (relative error means nothing next to a zero of the sine)
#   all four, as floats       equal to the correctly rounded float of the reference value on every input: no double-rounding case in the set
MEASURED_ABS_SINCOS_D = 1.4414467883194781e-16
MEASURED_ABS_ATAN_D = 1.691355389077387e-16
TOL_ABS_SINCOS_D = 4 * MEASURED_ABS_SINCOS_D
TOL_ABS_ATAN_D = 4 * MEASURED_ABS_ATAN_D
DOUBLE_ROUNDING = {}                                # fn -> (input, this header's float, the correctly rounded float); at most one per function
MATH_SINCOS_D, MATH_ATAN_D, MATH_SINCOS_F, MATH_ANGLE_F = 0, 1, 2, 3
PI_REF = 3.1415926


def _neighbours(centres, k=50):
    """each centre and its k nearest doubles on either side"""
    out = []
    for c in centres:
        lo = hi = np.float64(c)
        out.append(lo)
        for _ in range(k):
            lo = np.nextafter(lo, -np.inf); hi = np.nextafter(hi, np.inf)
            out += [lo, hi]
    return np.array(out, np.float64)


_math_cache = {}


def math_inputs(fn):
    """the probe's fixed inputs (doubles; for the float functions every value is a float), at least 10^6 per function, without NaN"""
    if fn in _math_cache:
        return _math_cache[fn]
    rs = np.random.RandomState(4000 + fn)
    headings = rs.uniform(-363, 363, 500_000).astype(np.float32)
    if fn == MATH_SINCOS_D:
        x = np.concatenate([rs.uniform(-3 * np.pi, 3 * np.pi, 1_000_000), _neighbours(np.arange(-12, 13) * (np.pi / 4)),
                            headings.astype(np.float64) / 180.0 * PI_REF,                     # what propose_move hands over
                            [0.0, -0.0, 3 * np.pi, -3 * np.pi, 5e-324, -5e-324, 1e-300, 1e-8]])
    elif fn == MATH_SINCOS_F:
        more = rs.uniform(-363, 363, 1_000_000).astype(np.float32)
        grid = np.arange(-362, 363, dtype=np.float32)
        near = np.stack([np.nextafter(grid, np.float32(-np.inf)), np.nextafter(grid, np.float32(np.inf))]).reshape(-1)   # every whole degree's two float neighbours
        x = np.concatenate([headings, more, grid, near, np.float32([0.0, -0.0, 1e-40, -1e-40])]).astype(np.float64)
    else:
        tx, ty = rs.uniform(-200, 200, (2, 500_000)).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            quot = (ty / tx).astype(np.float32)
        quot = quot[np.isfinite(quot)]
        mag = 10.0 ** rs.uniform(-300, 300, 300_000)
        x = np.concatenate([quot.astype(np.float64), mag, -mag, rs.uniform(-4, 4, 500_000),
                            _neighbours([0.4375, 0.6875, 1.1875, 2.4375, 0.5, 1.0, 1.5]), -_neighbours([0.4375, 0.6875, 1.1875, 2.4375, 0.5, 1.0, 1.5]),
                            [np.inf, -np.inf, 0.0, -0.0, np.finfo(np.float64).max, -np.finfo(np.float64).max, 5e-324, -5e-324]])
        if fn == MATH_ANGLE_F:                                                                 # the radar divides floats: every quotient is a float
            with np.errstate(over="ignore", under="ignore"):
                x = x.astype(np.float32).astype(np.float64)
    x = np.ascontiguousarray(x, np.float64)
    assert x.size >= 1_000_000 and not np.any(np.isnan(x))
    x.setflags(write=False)
    _math_cache[fn] = x
    return x


def fixture_maze():
    from dne_hip import _lib
    return _lib.load_maze(MAZE_FILE)


# ---- synthetic mazes: a bounding box and short segments inside it, none within 12 units of the start ---------------------------------------
def synthetic_maze(n_walls, seed=0):
    """(header8, lines [n_walls][4]).  n_walls = 1: one wall across the navigator's path; otherwise the box's four sides come first."""
    rs = np.random.RandomState(1000 + 31 * n_walls + seed)
    start, goal = (60.0, 100.0), (170.0, 30.0)
    header = np.array([0.0, 400.0, start[0], start[1], 0.0, goal[0], goal[1], 0.0], np.float32)
    if n_walls == 1:
        return header, np.array([[95.0, 20.0, 90.0, 180.0]], np.float32)
    lines = [[0, 0, 200, 3], [200, 3, 197, 200], [197, 200, 2, 198], [2, 198, 0, 0]][:n_walls]
    while len(lines) < n_walls:
        c = rs.uniform(10, 190, size=2)
        a = rs.uniform(0, 2 * np.pi)
        h = rs.uniform(4, 22)
        seg = [c[0] - h * np.cos(a), c[1] - h * np.sin(a), c[0] + h * np.cos(a), c[1] + h * np.sin(a)]
        # distance from the start to the segment
        p, q, s = np.array(seg[:2]), np.array(seg[2:]), np.array(start)
        u = np.clip(np.dot(s - p, q - p) / np.dot(q - p, q - p), 0, 1)
        if np.linalg.norm(p + u * (q - p) - s) < 12:
            continue
        lines.append([round(v, 2) for v in seg])
    return header, np.array(lines, np.float32)


# ---- thetas ------------------------------------------------------------------------------------------------------------------------------
def maze_noise(count=200_000, seed=77):
    return np.random.RandomState(seed).randn(count).astype(np.float32)


def theta0(noise, idx=1234):
    """TrainingState.initialize: noise.get(idx, P) * scale_by in fp32"""
    from dne_hip import policies
    return noise[idx:idx + P] * policies.simple_scale_by()


def perturbed(base, noise, off, scale):
    """theta_p = base_p + fl(scale * noise[off + p]): two fp32 roundings (csrc/maze.h: perturbed)"""
    return (np.asarray(base, np.float32) + np.float32(scale) * noise[off:off + P]).astype(np.float32)


def constant_action_theta(a0, a1):
    """every weight 0, the output biases the action: the policy answers (a0, a1) whatever it sees"""
    th = np.zeros(P, np.float32)
    th[B3], th[B3 + 1] = a0, a1
    return th


def straight_into_wall_theta():
    return constant_action_theta(0.0, 0.7)       # no turn, full speed ahead: into the first wall on the heading-0 ray, then pinned


def spin_in_place_theta():
    return constant_action_theta(0.7, 0.0)       # full turn rate, speed 0: the heading wraps through 360 every 120 steps


# ---- the policy in numpy --------------------------------------------------------------------------------------------------------------------
def fmaf32(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise.  The product of two floats is exact in double; the double sum s = p + c carries an
    exact error e (TwoSum); rounding s to float is right unless s sits exactly half way between two floats and e != 0 -- then e decides."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    up = np.nextafter(r, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(r, np.float32(-np.inf)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tie_up = (s - r64) * 2 == (up - r64)       # s is the midpoint of (r, up): the cast rounded to even, possibly the wrong way
        tie_dn = (r64 - s) * 2 == (r64 - dn)
    r = np.where(tie_up & (s != r64) & (e > 0), up.astype(np.float32), r)
    r = np.where(tie_dn & (s != r64) & (e < 0), dn.astype(np.float32), r)
    return r.astype(np.float32)


def dense_np(x, w, b):
    """[n_in] x [n_in][n_out] -> [n_out]: per unit one fmaf chain over k ascending from +0.0f, then + b"""
    acc = np.zeros(w.shape[1], np.float32)
    for k in range(w.shape[0]):
        acc = fmaf32(np.full(w.shape[1], x[k], np.float32), w[k], acc)
    return (acc + b).astype(np.float32)


def forward_np(theta, obs):
    th = np.asarray(theta, np.float32)
    relu = lambda v: np.where(v > 0, v, np.float32(0.0)).astype(np.float32)
    h1 = relu(dense_np(obs, th[W1:B1].reshape(11, 16), th[B1:W2]))
    h2 = relu(dense_np(h1, th[W2:B2].reshape(16, 16), th[B2:W3]))
    return h1, h2, dense_np(h2, th[W3:B3].reshape(16, 2), th[B3:P])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- dne_maze_rollout_host behind the Engine surface -------------------------------------------------------------------------------------------
class MazeHostEngine(OracleEngine):
    """The maze kind without a GPU: evaluations are dne_maze_rollout_host on thetas perturbed in numpy; ranks, the weighted sum and the
    optimizer are the oracle's (OracleEngine.es_update), as on every other kind."""

    def __init__(self, max_members=64, **kw):
        from dne_hip import _lib
        self.kind, self.n_actions, self.max_members, self.ref_count = _lib.KIND_MAZE, 2, max_members, 0
        self.P = P
        self.bc_max_steps, self.bc_final_only = kw.get("bc_max_steps", 0), False
        self.theta = np.zeros(P, np.float32)
        self.slots = {}
        self.noise = self.opt = self.members = self.maze = None
        self.calls = []

    def set_theta(self, theta, slot=0):
        if slot == 0:
            self.theta = np.array(theta, np.float32)
        self.slots[slot] = np.array(theta, np.float32)

    def maze_set_walls(self, header, lines):
        self.maze = (np.array(header, np.float32), np.array(lines, np.float32).reshape(-1, 4))

    def _run(self, thetas, tslimit):
        from dne_hip import _lib
        if self.maze is None:
            raise _lib.DneError("no maze loaded (maze_set_walls)")
        ret, ln, xy = _lib.maze_rollout_host(np.stack(thetas), self.maze[0], self.maze[1], tslimit)
        self._xy = xy
        return ret, np.sign(ret).astype(np.float32), ln

    def es_eval(self, idx, sigma, tslimit, seeds, want_bc=False):
        self.calls.append(("es_eval", len(idx)))
        th = [perturbed(self.theta, self.noise, int(i), s) for i in idx for s in (sigma, -sigma)]
        ret, sg, ln = self._run(th, tslimit)
        out = ret.reshape(-1, 2), sg.reshape(-1, 2), ln.reshape(-1, 2)
        self._last = (np.asarray(idx, np.int64),) + out
        return out

    def eval_members(self, n, tslimit, seeds, want_bc=False):
        slot, off, scale = self.members
        base = dict(self.slots); base[0] = self.theta
        return self._run([perturbed(base[int(slot[i])], self.noise, int(off[i]), scale[i]) for i in range(n)], tslimit)

    def maze_final_state(self, n):
        return self._xy[:n].copy()
