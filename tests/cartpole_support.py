"""TEST-ONLY support for gym.CartPole-v1 (DNE_KIND_CARTPOLE, csrc/cartpole.h): the contract in plain Python (a Python
float is an IEEE double; float32 through numpy; the forward pass through maze_support's fmaf32 chains; sine and cosine from
_lib.maze_math_host(0, .), the same sincos_d the header calls), the open-loop sequences and threshold states of the tests, member sets,
balancing_theta(), the measured distance to a libm version of the step, and CartPoleHostEngine -- dne_cartpole_rollout_host (the same header
compiled for the CPU) behind the Engine method surface, as maze_support.MazeHostEngine puts the maze's host twin behind it."""
import math

import numpy as np

from maze_support import dense_np, maze_noise   # noqa: F401 (maze_noise: the tests' 200 000-entry table)
from oracle_engine import OracleEngine

GAME = "gym.CartPole-v1"
P, OBS, STEPS = 386, 4, 500
W1, B1, W2, B2, W3, B3 = 0, 64, 80, 336, 352, 384
GRAVITY, MASSCART, MASSPOLE, LENGTH, FORCE_MAG, TAU = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
TOTAL_MASS = MASSPOLE + MASSCART
POLEMASS_LENGTH = MASSPOLE * LENGTH
X_TH = 2.4
TH = float.fromhex("0x1.acee9f37bebd5p-3")          # 12 * 2 * pi / 360
assert TH == 0.20943951023931953 == 12 * 2 * math.pi / 360

# seed 0 as the issue states it: the four splitmix64 outputs and the state they give
SEED0_R = (0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f, 0xf88bb8a8724c81ec)
SEED0_STATE = (0.03833108082136426, -0.006847200295149, -0.04735662284074023, 0.04708819781538286)

# ---- against libm: the step with math.sin / math.cos in place of sincos_d, over open_loop_cases() ------------------------------------------------
# Measured (glibc 2.35) over the seven sequences, every step up to and including each sequence's first done step (past it the pole falls
# through angles no episode sees): the largest absolute difference of any state value is MEASURED_LIBM = 0 -- on |theta| <= 0.21 sincos_d
# and glibc's correctly-rounded-in-practice sin / cos return the same doubles on every call made -- and every sequence ends at the same step.
# sincos_d and libm may differ by an ulp per call; a wrong formula shows as a difference many orders larger.  The bound is four times the
# measurement, as for the maze's state (maze_support.TOL_STATE).
MEASURED_LIBM = 0.0
TOL_LIBM = 4 * MEASURED_LIBM

M64 = (1 << 64) - 1


def splitmix_r(seed):
    """the four 64-bit outputs of splitmix64 from z = seed"""
    z, out = int(seed), []
    for _ in range(4):
        z = (z + 0x9E3779B97F4A7C15) & M64
        r = z
        r = ((r ^ (r >> 30)) * 0xBF58476D1CE4E5B9) & M64
        r = ((r ^ (r >> 27)) * 0x94D049BB133111EB) & M64
        r ^= r >> 31
        out.append(r)
    return out


def reset_py(seed):
    return [-0.05 + 0.1 * ((r >> 11) * 2.0 ** -53) for r in splitmix_r(seed)]


def sincos_header(theta):
    from dne_hip import _lib
    s, c = _lib.maze_math_host(0, [theta])[0]
    return float(s), float(c)


def sincos_libm(theta):
    return math.sin(theta), math.cos(theta)


def step_py(state, a, sincos=sincos_header):
    """one step in the issue's association; returns (new state, done)"""
    x, x_dot, theta, theta_dot = state
    force = FORCE_MAG if a == 1 else -FORCE_MAG
    s, c = sincos(theta)
    temp = (force + ((POLEMASS_LENGTH * theta_dot) * theta_dot) * s) / TOTAL_MASS
    thetaacc = (GRAVITY * s - c * temp) / (LENGTH * (4.0 / 3.0 - ((MASSPOLE * c) * c) / TOTAL_MASS))
    xacc = temp - ((POLEMASS_LENGTH * thetaacc) * c) / TOTAL_MASS
    new = [x + TAU * x_dot, x_dot + TAU * xacc, theta + TAU * theta_dot, theta_dot + TAU * thetaacc]
    done = new[0] < -X_TH or new[0] > X_TH or new[2] < -TH or new[2] > TH
    return new, done


def actions_py(actions, init, sincos=sincos_header):
    """rows [T][5] as dne_cartpole_actions_host: the state after each step, then done; stepping goes on past done"""
    state, rows = [float(v) for v in init], []
    for a in actions:
        state, done = step_py(state, int(a), sincos)
        rows.append(state + [1.0 if done else 0.0])
    return np.array(rows, np.float64)


def obs_of(state):
    return np.array(state, np.float64).astype(np.float32)


def forward_np(theta, obs):
    th = np.asarray(theta, np.float32)
    relu = lambda v: np.where(v > 0, v, np.float32(0.0)).astype(np.float32)
    h1 = relu(dense_np(obs, th[W1:B1].reshape(4, 16), th[B1:W2]))
    h2 = relu(dense_np(h1, th[W2:B2].reshape(16, 16), th[B2:W3]))
    return h1, h2, dense_np(h2, th[W3:B3].reshape(16, 2), th[B3:P])


def pick_action(out):
    return 1 if out[1] > out[0] else 0              # the first maximum on a tie; 0 when either logit is NaN


def rollout_py(theta, init, tslimit=STEPS, actions=None):
    """closed loop in plain Python with the float32 forward pass: (length, final state); the actions taken are appended to `actions`"""
    state, t = [float(v) for v in init], 0
    while t < min(tslimit, STEPS):
        a = pick_action(forward_np(theta, obs_of(state))[2])
        if actions is not None:
            actions.append(a)
        state, done = step_py(state, a)
        t += 1
        if done:
            break
    return t, state


def first_done(rows):
    """1-based step at which done first shows (the sequence's length if never)"""
    d = np.flatnonzero(rows[:, 4])
    return int(d[0]) + 1 if d.size else rows.shape[0]


_cases = None


def open_loop_cases():
    """[(name, actions int32 [T], init float64 [4])]: constant 0, constant 1 and alternating from the zero state, three random 0/1 sequences of
    500 from seeded resets -- the issue's six -- and one more that stays inside the thresholds for all of its 500 steps, so that the comparisons
    see a long episode too: the actions balancing_theta() takes from BALANCE_INIT"""
    global _cases
    if _cases is None:
        z = np.zeros(4)
        _cases = [("zeros", np.zeros(40, np.int32), z), ("ones", np.ones(40, np.int32), z), ("alternating", np.arange(40, dtype=np.int32) % 2, z)]
        for k, seed in enumerate((11, 2 ** 31 + 5, 2 ** 32 - 1)):
            _cases.append(("random%d" % k, np.random.RandomState(500 + k).randint(0, 2, 500).astype(np.int32), np.array(reset_py(seed))))
        acts = []
        rollout_py(balancing_theta(), BALANCE_INIT, actions=acts)
        _cases.append(("balanced", np.array(acts, np.int32), np.array(BALANCE_INIT)))
    return _cases


def threshold_states():
    """[(init, done after step 1)]: theta_dot = x_dot = 0, so the first step leaves theta and x where they are -- ON a threshold goes on, the
    next double beyond ends"""
    out = []
    for sign in (1.0, -1.0):
        out.append(([0.0, 0.0, sign * TH, 0.0], False))
        out.append(([0.0, 0.0, sign * math.nextafter(TH, 1.0), 0.0], True))
        out.append(([sign * X_TH, 0.0, 0.0, 0.0], False))
        out.append(([sign * math.nextafter(X_TH, 3.0), 0.0, 0.0, 0.0], True))
    return out


# ---- thetas ------------------------------------------------------------------------------------------------------------------------------
def theta0(noise, idx=1234):
    """TrainingState.initialize: noise.get(idx, P) * scale_by in fp32"""
    from dne_hip import _lib, policies
    return noise[idx:idx + P] * policies.simple_scale_by(_lib.KIND_CARTPOLE)


def perturbed(base, noise, off, scale):
    """theta_p = base_p + fl(scale * noise[off + p]): two fp32 roundings (csrc/maze.h: perturbed)"""
    return (np.asarray(base, np.float32) + np.float32(scale) * noise[off:off + P]).astype(np.float32)


BALANCE_W = (0.02, 0.1, 1.0, 0.5)
BALANCE_INIT = (0.03, -0.02, 0.04, 0.01)
BALANCE_FINAL_X = 1.2402981400520736                # the issue's float32-forward Python run from BALANCE_INIT: 500 steps, ending here


def balancing_theta():
    """fc1 unit 0 = w . obs and unit 1 = -w . obs, fc2 passes them through, out[1] = unit 0 and out[0] = unit 1: push right when w . obs > 0"""
    th = np.zeros(P, np.float32)
    for k, w in enumerate(BALANCE_W):
        th[W1 + k * 16 + 0], th[W1 + k * 16 + 1] = w, -w
    th[W2 + 0 * 16 + 0] = th[W2 + 1 * 16 + 1] = 1.0
    th[W3 + 0 * 2 + 1] = th[W3 + 1 * 2 + 0] = 1.0
    return th


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- dne_cartpole_rollout_host behind the Engine surface ---------------------------------------------------------------------------------------
class CartPoleHostEngine(OracleEngine):
    """The cart-pole kind without a GPU: evaluations are dne_cartpole_rollout_host on thetas perturbed in numpy, each under its own
    environment seed; ranks, the weighted sum and the optimizer are the oracle's (OracleEngine.es_update), as on every other kind."""

    def __init__(self, max_members=64, **kw):
        from dne_hip import _lib
        self.kind, self.n_actions, self.max_members, self.ref_count = _lib.KIND_CARTPOLE, 2, max_members, 0
        self.P = P
        self.bc_max_steps, self.bc_final_only = 0, False
        self.theta = np.zeros(P, np.float32)
        self.slots = {}
        self.noise = self.opt = self.members = None
        self.calls = []
        self.seeds_seen = []

    def set_theta(self, theta, slot=0):
        if slot == 0:
            self.theta = np.array(theta, np.float32)
        self.slots[slot] = np.array(theta, np.float32)

    def _run(self, thetas, tslimit, seeds):
        from dne_hip import _lib
        seeds = np.asarray(seeds, np.uint32).reshape(-1)
        self.seeds_seen.append(seeds.copy())
        ret, ln, state = _lib.cartpole_rollout_host(np.stack(thetas), seeds, tslimit)
        self._state = state
        return ret, ret.copy(), ln

    def es_eval(self, idx, sigma, tslimit, seeds, want_bc=False):
        self.calls.append(("es_eval", len(idx)))
        th = [perturbed(self.theta, self.noise, int(i), s) for i in idx for s in (sigma, -sigma)]
        ret, sg, ln = self._run(th, tslimit, seeds)
        out = ret.reshape(-1, 2), sg.reshape(-1, 2), ln.reshape(-1, 2)
        self._last = (np.asarray(idx, np.int64),) + out
        return out

    def eval_members(self, n, tslimit, seeds, want_bc=False):
        slot, off, scale = self.members
        base = dict(self.slots); base[0] = self.theta
        return self._run([perturbed(base[int(slot[i])], self.noise, int(off[i]), scale[i]) for i in range(n)], tslimit, seeds[:n])

    def cartpole_final_state(self, n):
        return self._state[:n].copy()
