"""TEST-ONLY support for MujocoPolicy on the pendulum (DNE_KIND_PENDULUM, csrc/pendulum.h): the contract in plain Python (a
Python float is an IEEE double; float32 through numpy; the dense layers through maze_support's fmaf32 in the four-chain association; sine and
cosine from _lib.maze_math_host(0, .) and tanh from _lib.pendulum_math_host('tanh', .), the same functions the header calls -- tanh_f has a
test of its own against libm), the textbook step in gym's own form, the open-loop sequences of the tests, the measured distances, and
PendulumHostEngine -- dne_pendulum_rollout_host (the same header compiled for the CPU) behind the Engine method surface."""
import math

import numpy as np

from maze_support import fmaf32, maze_noise   # noqa: F401 (maze_noise: the tests' 200 000-entry table)
from oracle_engine import OracleEngine

ENV_ID = "Pendulum-v0"
OBS, STEPS = 3, 200
PI, TWO_PI = math.pi, 2 * math.pi
assert PI == 3.141592653589793 and TWO_PI == 6.283185307179586
DT, MAX_SPEED, MAX_TORQUE = 0.05, 8.0, 2.0

# ---- measured distances (glibc 2.35), each over every step of open_loop_cases() -----------------------------------------------------------------
# Against gym's own form, ONE step at a time (step_gym on the twin's previous state against the twin's next state and reward): the largest
# absolute difference of theta / theta_dot after the step, and of the float32 reward.  The contract differs from the textbook in how the angle
# is normalised (floor instead of %), in sin(norm(theta)) for sin(theta + pi) negated, in sincos_d for libm and in the association of the cost;
# each is worth a few ulps of a value of magnitude <= 90, a wrong formula shows many orders above.  The bound is four times the measurement
# (the margin maze_support.TOL_STATE and cartpole_support.TOL_LIBM take).
MEASURED_GYM_STATE = 5.329070518200751e-15     # (6 ulps of a theta near 5; theta reaches +-75 in these sequences)
MEASURED_GYM_REWARD = 0.0                      # every one of the 2200 float32 rewards is the same float
TOL_GYM_STATE, TOL_GYM_REWARD = 4 * MEASURED_GYM_STATE, 4 * MEASURED_GYM_REWARD
# The contract's return (float rewards summed as doubles in step order, one cast) against numpy's pairwise float32 rews.sum() over the same
# episodes: the largest absolute difference; the bound is twice it.
MEASURED_SUM = 0.0001220703125                  # 2^-13: one float32 ulp of a return between -1024 and -2048
TOL_SUM = 2 * MEASURED_SUM

M64 = (1 << 64) - 1


def offsets(H, O):
    w1, b1 = 0, OBS * H
    w2 = b1 + H
    b2 = w2 + H * H
    w3 = b2 + H
    b3 = w3 + H * O
    return w1, b1, w2, b2, w3, b3, b3 + O


def splitmix_r(seed, n=2):
    """the first n 64-bit outputs of splitmix64 from z = seed"""
    z, out = int(seed), []
    for _ in range(n):
        z = (z + 0x9E3779B97F4A7C15) & M64
        r = z
        r = ((r ^ (r >> 30)) * 0xBF58476D1CE4E5B9) & M64
        r = ((r ^ (r >> 27)) * 0x94D049BB133111EB) & M64
        r ^= r >> 31
        out.append(r)
    return out


def reset_py(seed):
    u0, u1 = ((r >> 11) * 2.0 ** -53 for r in splitmix_r(seed))
    return [-PI + TWO_PI * u0, -1.0 + 2.0 * u1]


def norm_py(x):
    return x - TWO_PI * math.floor((x + PI) / TWO_PI)


def sincos_header(x):
    from dne_hip import _lib
    s, c = _lib.maze_math_host(0, [x])[0]
    return float(s), float(c)


def tanh_header(v):
    from dne_hip import _lib
    return _lib.pendulum_math_host('tanh', np.asarray(v, np.float32).astype(np.float64)).astype(np.float32)


def obs_py(state):
    s, c = sincos_header(norm_py(state[0]))
    return np.array([c, s, state[1]], np.float64).astype(np.float32)


def step_py(state, a):
    """one step in the issue's association under the float32 action a; returns (new state, float32 reward)"""
    th, thdot = state
    a = np.float32(a)
    u = -2.0 if a < -2 else (2.0 if a > 2 else float(a))
    n = norm_py(th)
    s, _ = sincos_header(n)
    cost = (n * n + 0.1 * (thdot * thdot)) + 0.001 * (u * u)
    nd = thdot + (15.0 * s + 3.0 * u) * DT
    nth = th + nd * DT
    nd = -MAX_SPEED if nd < -MAX_SPEED else (MAX_SPEED if nd > MAX_SPEED else nd)
    return [nth, nd], np.float32(-cost)


def step_gym(state, a):
    """the textbook step as gym's classic_control/pendulum.py writes it (libm, %, np.clip); returns (new state, reward as a double)"""
    th, thdot = state
    g, m, l = 10.0, 1.0, 1.0
    u = float(np.clip(float(np.float32(a)), -MAX_TORQUE, MAX_TORQUE))
    costs = (((th + math.pi) % (2 * math.pi)) - math.pi) ** 2 + .1 * thdot ** 2 + .001 * (u ** 2)
    newthdot = thdot + (-3 * g / (2 * l) * math.sin(th + math.pi) + 3. / (m * l ** 2) * u) * DT
    newth = th + newthdot * DT
    newthdot = float(np.clip(newthdot, -MAX_SPEED, MAX_SPEED))
    return [newth, newthdot], -costs


def actions_py(actions, init):
    """rows [T][3] as dne_pendulum_actions_host: theta and theta_dot after each step, then the reward"""
    state, rows = [float(v) for v in init], []
    for a in actions:
        state, rew = step_py(state, a)
        rows.append(state + [float(rew)])
    return np.array(rows, np.float64)


def return_py(rews32):
    """(return, sign return) of float32 rewards: summed as doubles in step order, cast once"""
    ret = sg = 0.0
    for r in rews32:
        ret += float(r)
        sg += float(np.sign(np.float32(r)))
    return np.float32(ret), np.float32(sg)


_cases = None


def open_loop_cases():
    """[(name, actions float32 [200], init float64 [2])]: constant +2, constant -2, zero, alternating +-2 from the resets of seeds 0 and 1,
    and three seeded random sequences in [-3, 3] (so that the clip is exercised) from the resets of 2^31, 2^32 - 1 and 7"""
    global _cases
    if _cases is None:
        _cases = []
        for k, seed in enumerate((0, 1)):
            init = np.array(reset_py(seed))
            _cases += [("plus2_%d" % k, np.full(STEPS, 2.0, np.float32), init), ("minus2_%d" % k, np.full(STEPS, -2.0, np.float32), init),
                       ("zero_%d" % k, np.zeros(STEPS, np.float32), init),
                       ("alternating_%d" % k, np.where(np.arange(STEPS) % 2 == 0, 2.0, -2.0).astype(np.float32), init)]
        for k, seed in enumerate((2 ** 31, 2 ** 32 - 1, 7)):
            _cases.append(("random%d" % k, np.random.RandomState(900 + k).uniform(-3, 3, STEPS).astype(np.float32), np.array(reset_py(seed))))
    return _cases


# ---- the policy ------------------------------------------------------------------------------------------------------------------------------
def dense4_np(x, w, b):
    """[n_in] x [n_in][n_out] -> [n_out]: per unit four fmaf chains over k = r (mod 4) ascending from +0.0f, ((c0 + c1) + (c2 + c3)) + b"""
    c = [np.zeros(w.shape[1], np.float32) for _ in range(4)]
    for k in range(w.shape[0]):
        c[k & 3] = fmaf32(np.full(w.shape[1], x[k], np.float32), w[k], c[k & 3])
    return (((c[0] + c[1]).astype(np.float32) + (c[2] + c[3]).astype(np.float32)).astype(np.float32) + np.asarray(b, np.float32)).astype(np.float32)


def normalise_np(ob, mean, std):
    with np.errstate(all="ignore"):
        x = ((np.asarray(ob, np.float32) - np.asarray(mean, np.float32)).astype(np.float32) / np.asarray(std, np.float32)).astype(np.float32)
    return np.where(x < -5, np.float32(-5), np.where(x > 5, np.float32(5), x)).astype(np.float32)


def pick_action_np(out, mode):
    if mode == 'continuous':
        return np.float32(out[0])
    aidx, best = 0, np.float32(-np.inf)
    for i, v in enumerate(out):
        if v > best:
            best, aidx = v, i
    B = np.float32(len(out))
    return np.float32(np.float32(np.float32(np.float32(1.0) / np.float32(B - np.float32(1.0))) * np.float32(aidx)) * np.float32(4.0) + np.float32(-2.0))


def forward_np(theta, ob, H, O, mode, nonlin, mean, std):
    """-> (x, h1, h2, out, action) as dne_pendulum_forward_host"""
    th = np.asarray(theta, np.float32)
    w1, b1, w2, b2, w3, b3, P = offsets(H, O)
    nl = tanh_header if nonlin == 'tanh' else (lambda v: np.where(v > 0, v, np.float32(0.0)).astype(np.float32))
    x = normalise_np(ob, mean, std)
    h1 = nl(dense4_np(x, th[w1:b1].reshape(OBS, H), th[b1:w2]))
    h2 = nl(dense4_np(h1, th[w2:b2].reshape(H, H), th[b2:w3]))
    out = dense4_np(h2, th[w3:b3].reshape(H, O), th[b3:P])
    return x, h1, h2, out, pick_action_np(out, mode)


def perturbed(base, noise, off, scale):
    """theta_p = base_p + fl(scale * noise[off + p]): two fp32 roundings (csrc/maze.h: perturbed)"""
    base = np.asarray(base, np.float32)
    return (base + np.float32(scale) * noise[off:off + base.size]).astype(np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def humanoid_exp(pop=8, calc_obstat_prob=0.5, ac_noise_std=0.01, eval_prob=1.0, hidden=64, ac_bins="continuous:", nonlin="tanh", env_id=ENV_ID):
    """configurations/humanoid.json with "env_id": "Pendulum-v0", at a test's size"""
    return {"config": {"calc_obstat_prob": calc_obstat_prob, "episodes_per_batch": pop, "eval_prob": eval_prob, "l2coeff": 0.005, "noise_stdev": 0.02,
                       "snapshot_freq": 0, "timesteps_per_batch": 10, "return_proc_mode": "centered_rank", "episode_cutoff_mode": "env_default"},
            "env_id": env_id, "exp_prefix": "humanoid", "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"},
            "policy": {"args": {"ac_bins": ac_bins, "ac_noise_std": ac_noise_std, "connection_type": "ff", "hidden_dims": [hidden, hidden],
                                "nonlin_type": nonlin}, "type": "MujocoPolicy"}}


# ---- dne_pendulum_rollout_host behind the Engine surface ---------------------------------------------------------------------------------------
class PendulumHostEngine(OracleEngine):
    """The pendulum kind without a GPU: evaluations are dne_pendulum_rollout_host on thetas perturbed in numpy, each under its own environment
    seed, with the options and statistics calls of the device engine; ranks, the weighted sum and the optimizer are the oracle's."""

    def __init__(self, hidden=64, n_out=1, ac_mode='continuous', nonlin='tanh', max_members=64, **kw):
        from dne_hip import _lib
        self.kind, self.n_actions, self.max_members, self.ref_count = _lib.KIND_PENDULUM, n_out, max_members, 0
        self.hidden, self.ac_mode, self.nonlin = hidden, ac_mode, nonlin
        self.P = _lib.pendulum_num_params(hidden, n_out)
        self.bc_max_steps, self.bc_final_only = 0, False
        self.theta = np.zeros(self.P, np.float32)
        self.slots = {}
        self.noise = self.opt = self.members = None
        self.mean = self.std = None
        self.options = None
        self.calls, self.seeds_seen, self.options_seen, self.ob_stats_seen = [], [], [], []

    def set_theta(self, theta, slot=0):
        if slot == 0:
            self.theta = np.array(theta, np.float32)
        self.slots[slot] = np.array(theta, np.float32)

    def pendulum_set_ob_stat(self, mean, std):
        self.mean, self.std = np.array(mean, np.float32), np.array(std, np.float32)
        self.ob_stats_seen.append((self.mean.copy(), self.std.copy()))

    def pendulum_set_rollout_options(self, n, ac_noise_std=0.0, ac_off=None, stat_flag=None):
        from dne_hip import _lib
        if ac_off is not None and (np.asarray(ac_off) + STEPS > self.noise.size).any():
            raise _lib.DneError("dne_pendulum_set_rollout_options: an action-noise offset reaches past the noise table")
        self.options = (int(n), float(ac_noise_std), None if ac_off is None else np.array(ac_off, np.int64),
                        None if stat_flag is None else np.array(stat_flag, np.uint8))
        self.options_seen.append(self.options)

    def _run(self, thetas, tslimit, seeds):
        from dne_hip import _lib
        if self.mean is None:
            raise _lib.DneError("the observation statistics of a DNE_KIND_PENDULUM engine are NaN until dne_pendulum_set_ob_stat is called")
        seeds = np.asarray(seeds, np.uint32).reshape(-1)
        self.seeds_seen.append(seeds.copy())
        n, std, off, flag = self.options or (len(thetas), 0.0, None, None)
        assert n == len(thetas), "the rollout options were given for %d members, the evaluation runs %d" % (n, len(thetas))
        self.options = None                      # for the next evaluation only
        r = _lib.pendulum_rollout_host(np.stack(thetas), seeds, self.hidden, self.mean, self.std, n_out=self.n_actions, ac_mode=self.ac_mode,
                                       nonlin=self.nonlin, tslimit=tslimit, ac_noise_std=std, table=self.noise if off is not None else None,
                                       ac_off=off, stat_flag=flag)
        self._last_run = r
        return r['returns'], r['signreturns'], r['lengths']

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

    def pendulum_ob_stats(self, n):
        r = self._last_run
        return r['ob_sum'][:n].copy(), r['ob_sumsq'][:n].copy(), r['ob_count'][:n].copy()

    def pendulum_final_state(self, n):
        return self._last_run['state'][:n].copy()
