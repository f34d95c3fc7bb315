"""TEST-ONLY support for the hard maze (DNE_KIND_MAZE, csrc/maze.h): the fixtures, the tolerances of the comparison with the reference's
recording, synthetic mazes, member sets, a float32 numpy statement of the policy, and MazeHostEngine -- dne_maze_rollout_host (the same
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
