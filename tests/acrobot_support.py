"""TEST-ONLY support for gym.Acrobot-v1 (DNE_ENV_ACROBOT, csrc/acrobot.h): the contract in plain Python (a Python float is
an IEEE double; sine and cosine from _lib.maze_math_host(0, .) on the normalised argument, the same sincos_d(norm_angle(x)) the header calls), a
second restatement with libm in gym's own spelling (cos(x - pi/2), the wrap loops), the open-loop sequences, hand-placed states and member sets
of the tests, and AcrobotHostEngine -- dne_dense_rollout_host and the step twins on environment id 9 behind the Engine method surface, as
dense_gans_support.DenseGaNsHostEngine puts them behind it for the three engine kinds.  Every comparison with the twin is bit for bit."""
import math

import numpy as np

import dense_gans_support as GN
import dense_support as D
import stepenv_support as SS
from stepenv_support import bits, same   # noqa: F401 (re-exported)

GAME = "gym.Acrobot-v1"
ENV, OBS, ACT, S, STEPS = 9, 6, 3, 4, 500
PI, TWO_PI = 3.141592653589793, 6.283185307179586
M1 = M2 = 1.0
L1 = 1.0
LC1 = LC2 = 0.5
I1 = I2 = 1.0
G, DT = 9.8, 0.2
MAX_VEL_1, MAX_VEL_2 = 4.0 * PI, 9.0 * PI
# the constant factors, each in the association the header writes down
K_D1, K_LL, K_2LL, K_D2, K_LLC = M1 * (LC1 * LC1), L1 * L1 + LC2 * LC2, (2.0 * L1) * LC2, LC2 * LC2, L1 * LC2
K_PHI2, K_T1, K_T2, K_T3 = (M2 * LC2) * G, (M2 * L1) * LC2, ((2.0 * M2) * L1) * LC2, (M1 * LC1 + M2 * L1) * G
K_DEN, HALF_DT, SIXTH_DT = M2 * (LC2 * LC2) + I2, DT / 2.0, DT / 6.0

SEED0_STATE = (0.07666216164272852, -0.013694400590298, -0.09471324568148046, 0.09417639563076571)   # the issue's
# the issue's anchors: from (0, 0, 0, 0) under actions 2, 2, 0, computed with libm in gym's spelling
ANCHOR_ACTIONS = (2, 2, 0)
ANCHORS = ((-0.013262967177227795, 0.03428722934738544, -0.12866185280996106, 0.33450108998660194),
           (-0.0484896538093726, 0.12748779480535294, -0.2132848732767469, 0.5754630640496233),
           (-0.06723706338620503, 0.18553771278886602, 0.030714304370452555, -0.0064477093097422555))

# ---- against libm, in gym's spelling ---------------------------------------------------------------------------------------------------------------
# Measured (glibc 2.35) over every state the four open-loop sequences of open_loop_cases() visit (4 x 500 states, each stepped ONCE by both
# versions from the same state, under the sequence's own action: the system is chaotic, trajectories are not compared): the largest absolute
# difference of any state value after the step is MEASURED_LIBM.  The two versions differ by an ulp per sine / cosine call (cos(x - pi/2) against
# sin(x) besides), by the wrap at +-pi (excluded: an angle gym keeps at pi is -pi here, which is the same angle) and by nothing else; a wrong
# formula shows as 1e-3 or more.  The bound is four times the measurement, the project's convention (maze_support.TOL_STATE,
# cartpole_support.TOL_LIBM).
MEASURED_LIBM = 8.881784197001252e-16
TOL_LIBM = 4 * MEASURED_LIBM

M64 = (1 << 64) - 1


# ---- the contract ------------------------------------------------------------------------------------------------------------------------------------
def reset_py(seed):
    """cartpole's stream: four splitmix64 draws from z = seed, v = -0.1 + 0.2 * u"""
    z, out = int(seed), []
    for _ in range(4):
        z = (z + 0x9E3779B97F4A7C15) & M64
        r = z
        r = ((r ^ (r >> 30)) * 0xBF58476D1CE4E5B9) & M64
        r = ((r ^ (r >> 27)) * 0x94D049BB133111EB) & M64
        r ^= r >> 31
        out.append(-0.1 + 0.2 * ((r >> 11) * 2.0 ** -53))
    return out


def norm_angle(x):
    """pendulum.h's floor form; a NaN or an infinity gives NaN (floor passes both on, and inf - inf is NaN)"""
    if not math.isfinite(x):
        return float("nan")
    return x - TWO_PI * float(math.floor((x + PI) / TWO_PI))


def sc(x):
    """(sin, cos) as the header forms every one of them: sincos_d(norm_angle(x))"""
    from dne_hip import _lib
    s, c = _lib.maze_math_host(0, [norm_angle(x)])[0]
    return float(s), float(c)


def deriv_py(s, tau):
    th1, th2, w1, w2 = s
    s2, c2 = sc(th2)
    d1 = ((K_D1 + M2 * (K_LL + K_2LL * c2)) + I1) + I2
    d2 = M2 * (K_D2 + K_LLC * c2) + I2
    phi2 = K_PHI2 * sc(th1 + th2)[0]
    phi1 = (((-K_T1 * (w2 * w2)) * s2 - ((K_T2 * w2) * w1) * s2) + K_T3 * sc(th1)[0]) + phi2
    dw2 = (((tau + (d2 / d1) * phi1) - (K_T1 * (w1 * w1)) * s2) - phi2) / (K_DEN - (d2 * d2) / d1)
    dw1 = -(d2 * dw2 + phi1) / d1
    return [w1, w2, dw1, dw2]


def terminal_value(s):
    """-cos(th1) - cos(th2 + th1): terminal when > 1.0"""
    return -sc(s[0])[1] - sc(s[1] + s[0])[1]


def step_py(state, a):
    """one RK4 step in the header's association; returns (new state, terminal)"""
    s = [float(v) for v in state]
    tau = float(a - 1)
    nudged = lambda h, k: [s[i] + h * k[i] for i in range(4)]
    k1 = deriv_py(s, tau)
    k2 = deriv_py(nudged(HALF_DT, k1), tau)
    k3 = deriv_py(nudged(HALF_DT, k2), tau)
    k4 = deriv_py(nudged(DT, k3), tau)
    n = [s[i] + SIXTH_DT * (((k1[i] + 2.0 * k2[i]) + 2.0 * k3[i]) + k4[i]) for i in range(4)]
    n[0], n[1] = norm_angle(n[0]), norm_angle(n[1])
    for i, m in ((2, MAX_VEL_1), (3, MAX_VEL_2)):           # comparisons that let a NaN through
        if n[i] < -m:
            n[i] = -m
        if n[i] > m:
            n[i] = m
    return n, terminal_value(n) > 1.0


def obs_py(state):
    (s1, c1), (s2, c2) = sc(state[0]), sc(state[1])
    return np.array([c1, s1, c2, s2, state[2], state[3]], np.float64).astype(np.float32)


def pick_action(out):
    a = 0
    if out[1] > out[a]:
        a = 1
    if out[2] > out[a]:
        a = 2
    return a


def actions_py(actions, init):
    """rows [T][5] as dne_acrobot_actions_host: the state after each step, then terminal; stepping goes on past it"""
    state, rows = [float(v) for v in init], []
    for a in actions:
        state, over = step_py(state, int(a))
        rows.append(state + [1.0 if over else 0.0])
    return np.array(rows, np.float64)


# ---- the libm restatement, in gym's spelling ------------------------------------------------------------------------------------------------------------
def wrap_gym(x, m, M):
    if not math.isfinite(x):
        return x
    diff = M - m
    while x > M:
        x = x - diff
    while x < m:
        x = x + diff
    return x


def dsdt_gym(s, a):
    from math import cos, sin, pi
    m1, m2, l1, lc1, lc2, g = M1, M2, L1, LC1, LC2, G
    theta1, theta2, dtheta1, dtheta2 = s
    d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * cos(theta2)) + I1 + I2
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * cos(theta2)) + I2
    phi2 = m2 * lc2 * g * cos(theta1 + theta2 - pi / 2.)
    phi1 = - m2 * l1 * lc2 * dtheta2 ** 2 * sin(theta2) - 2 * m2 * l1 * lc2 * dtheta2 * dtheta1 * sin(theta2) \
        + (m1 * lc1 + m2 * l1) * g * cos(theta1 - pi / 2) + phi2
    ddtheta2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * dtheta1 ** 2 * sin(theta2) - phi2) / (m2 * lc2 ** 2 + I2 - d2 ** 2 / d1)
    ddtheta1 = -(d2 * ddtheta2 + phi1) / d1
    return np.array([dtheta1, dtheta2, ddtheta1, ddtheta2])


def step_libm(state, a):
    """gym's step: rk4 over [0, dt], wrap, bound; (new state, terminal).  Finite inputs only"""
    y0, torque, dt2 = np.array(state, np.float64), float(a - 1), DT / 2.0
    k1 = dsdt_gym(y0, torque)
    k2 = dsdt_gym(y0 + dt2 * k1, torque)
    k3 = dsdt_gym(y0 + dt2 * k2, torque)
    k4 = dsdt_gym(y0 + DT * k3, torque)
    ns = (y0 + DT / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)).tolist()
    ns[0], ns[1] = wrap_gym(ns[0], -math.pi, math.pi), wrap_gym(ns[1], -math.pi, math.pi)
    ns[2], ns[3] = min(max(ns[2], -MAX_VEL_1), MAX_VEL_1), min(max(ns[3], -MAX_VEL_2), MAX_VEL_2)
    return ns, bool(-math.cos(ns[0]) - math.cos(ns[1] + ns[0]) > 1.0)


def same_nan(a, b):
    """same(), with a NaN equal to a NaN whatever its sign and payload: a NaN an operation makes (inf - inf) is -NaN on x86 and +NaN elsewhere"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(np.where(na, 0, a).astype(a.dtype)), bits(np.where(nb, 0, b).astype(b.dtype)))


def angle_gap(a, b):
    """|a - b| of two angles, an angle at pi and one at -pi being the same angle"""
    d = abs(a - b)
    return min(d, abs(d - TWO_PI))


def state_gap(a, b):
    return max(angle_gap(a[0], b[0]), angle_gap(a[1], b[1]), abs(a[2] - b[2]), abs(a[3] - b[3]))


# ---- the tests' inputs ---------------------------------------------------------------------------------------------------------------------------------
def open_loop_cases():
    """(name, actions int32 [500], initial state): all 0, all 2, alternating 0 / 2, RandomState(1) over {0, 1, 2}"""
    rs = np.random.RandomState(1)
    init = np.array(reset_py(0))
    return (("all0", np.zeros(STEPS, np.int32), init), ("all2", np.full(STEPS, 2, np.int32), init),
            ("alternating", np.tile(np.array([0, 2], np.int32), STEPS // 2), init), ("random", rs.randint(0, 3, STEPS).astype(np.int32), init))


def ulp_steps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, math.inf if k > 0 else -math.inf)
    return float(x)


def edge_states():
    """hand-placed states: the angles at +-pi, each velocity at its clamp and one ulp inside it (both signs), a fast state whose RK4 arguments
    leave sincos_d's own range, a NaN, an infinity"""
    out = [(PI, 0.0, 0.0, 0.0), (-PI, 0.0, 0.0, 0.0), (0.0, PI, 0.0, 0.0), (0.0, -PI, 0.0, 0.0), (PI, PI, 0.5, -0.5), (-PI, -PI, -0.5, 0.5)]
    for sgn in (1.0, -1.0):
        for inside in (0, 1):
            out.append((0.3, -0.2, sgn * ulp_steps(MAX_VEL_1, -inside), 0.0))
            out.append((0.3, -0.2, 0.0, sgn * ulp_steps(MAX_VEL_2, -inside)))
            out.append((-2.0, 2.5, sgn * ulp_steps(MAX_VEL_1, -inside), -sgn * ulp_steps(MAX_VEL_2, -inside)))
    out.append((3.0, 3.1, MAX_VEL_1, MAX_VEL_2))
    out.append((float("nan"), 0.0, 0.0, 0.0))
    out.append((0.0, 0.0, float("nan"), 0.0))
    out.append((float("inf"), 0.0, 0.0, 0.0))
    return [tuple(float(v) for v in s) for s in out]


def threshold_states(span=400, th1s=(2.0, 1.9, 2.1, 1.8, 2.2, 1.95, 2.05)):
    """states at rest (th1, th2, 0, 0) whose step under action 1 lands ON the terminal threshold and one ulp either side of it: th2 is bisected
    (on the twin's own step) to where -cos(th1') - cos(th1' + th2') crosses 1.0, then scanned ulp by ulp -- an ulp of th2 near 0.15 moves the
    value by less than an ulp of 1.0, so a scan meets the doubles around the threshold (the step's own rounding can skip one: the next th1 of th1s is
    scanned for what is still missing).  -> {'equal' | 'below' | 'above': state}; a key is
    missing if the scan never produced that value (the test asserts all three are there)"""
    from dne_hip import _lib

    def values(th2s):
        init = np.array([[th1, th2, 0.0, 0.0] for th2 in th2s])
        rows = _lib.acrobot_actions_host(np.ones((len(th2s), 1), np.int32), init)[:, 0]
        return [terminal_value(r[:4]) for r in rows]

    want = {"equal": 1.0, "below": float(np.nextafter(1.0, 0.0)), "above": float(np.nextafter(1.0, 2.0))}
    found = {}
    for th1 in th1s:
        lo, hi = 0.0, 0.6
        vlo, vhi = values([lo, hi])
        assert vlo < 1.0 < vhi or vhi < 1.0 < vlo
        up = vhi > vlo
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if (values([mid])[0] > 1.0) == up:
                hi = mid
            else:
                lo = mid
        th2s = [ulp_steps(lo, -span)]
        for _ in range(2 * span):
            th2s.append(float(np.nextafter(th2s[-1], math.inf)))
        for th2, v in zip(th2s, values(th2s)):
            for name, w in want.items():
                if v == w and name not in found:
                    found[name] = (th1, th2, 0.0, 0.0)
        if len(found) == len(want):
            break
    return found


def theta_linear(W, b):
    """a LinearClassifier's flat vector: w [6][3] row-major, then b [3]"""
    return np.concatenate([np.asarray(W, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)]).astype(np.float32)


def solver_theta():
    """'torque follows omega2': W[5][0] = -1, W[5][2] = +1, b[1] = -1e-3, everything else 0"""
    W, b = np.zeros((6, 3), np.float32), np.zeros(3, np.float32)
    W[5, 0], W[5, 2], b[1] = -1.0, 1.0, -1e-3
    return theta_linear(W, b)


def zero_theta(P=21):
    return np.zeros(P, np.float32)


def random_members(n=200):
    """n LinearClassifier members: W, b = RandomState(0).randn(6, 3), randn(3) drawn alternately; member i runs under seed i"""
    rs = np.random.RandomState(0)
    th = []
    for _ in range(n):
        W = rs.randn(6, 3)
        th.append(theta_linear(W, rs.randn(3)))
    return np.stack(th), np.arange(n, dtype=np.uint32)


def num_params(hidden):
    d = (OBS,) + tuple(hidden) + (ACT,)
    return sum((d[l] + 1) * d[l + 1] for l in range(len(d) - 1))


def forward_np(hidden, nonlin, theta, obs):
    """dense_support.forward_np's chains on the acrobot's widths: (layers, out)"""
    D.N_IN.setdefault("acrobot", OBS); D.N_OUT.setdefault("acrobot", ACT)
    return D.forward_np("acrobot", hidden, nonlin, theta, obs)


def rollout(thetas, hidden, nonlin, seeds, tslimit=0, init=None):
    from dne_hip import _lib
    return _lib.dense_rollout_host(np.asarray(thetas, np.float32), ENV, hidden, nonlin, ACT, seeds=seeds, tslimit=tslimit, init=init)


def traces(thetas, hidden, nonlin, seeds, tslimit=0):
    """the episodes of n members in lock step on the twins (dne_dense_forward_host + dne_stepenv_step_host on the whole batch; a done environment
    keeps every bit): dict(states [T + 1][n][4] with the reset first, lengths [n], returns [n] -- the float64 sum of the rewards cast once)"""
    from dne_hip import _lib
    thetas = np.asarray(thetas, np.float32)
    batch = _lib.stepenv_reset_host(ENV, len(thetas), seeds, tslimit)
    states, total = [batch[0].copy()], np.zeros(len(thetas), np.float64)
    while not batch[3].all():
        _, _, a = _lib.dense_forward_host(thetas, batch[4], ENV, hidden, nonlin, ACT)
        total += _lib.stepenv_step_host(ENV, a, *batch).astype(np.float64)
        states.append(batch[0].copy())
    return dict(states=np.array(states), lengths=batch[1].copy(), returns=total.astype(np.float32))


# ---- the engine surface without a GPU -------------------------------------------------------------------------------------------------------------------
SHAPES = (((), "relu"), ((16, 16), "relu"), ((5, 33), "tanh"), ((64, 64, 64), "relu"))


class AcrobotHostEngine(GN.DenseGaNsHostEngine):
    """_lib.Engine's surface for a KIND_DENSE engine created on ENV_ACROBOT, over the CPU twins: DenseGaNsHostEngine's methods (episodes through
    dne_dense_rollout_host, the bank, BCs, archive, both novelty forms, update_support's update) with the attributes its constructors would set
    for a named kind set here for the environment id, which those constructors do not know"""

    def __init__(self, hidden=(), nonlin="relu", max_members=16, **kw):
        from dne_hip import _lib
        self.env = "acrobot"
        self.kind, self.env_kind = _lib.KIND_DENSE, _lib.ENV_ACROBOT
        self.hidden, self.nonlin_name, self.nonlin = tuple(int(w) for w in hidden), nonlin, _lib.DENSE_NONLINS[nonlin]
        self.n_actions, self.max_members, self.ref_count = ACT, int(max_members), 0
        self.P = _lib.dense_num_params(self.env_kind, self.hidden, self.n_actions)
        assert self.P == num_params(self.hidden)
        self.bc_max_steps, self.bc_final_only = 0, False
        self.slots = {0: np.zeros(self.P, np.float32)}
        self.noise = self.members = None
        self.m, self.v, self.t = np.zeros(self.P, np.float32), np.zeros(self.P, np.float32), 0
        self.envs = SS.StepEnvHostEngine(self.env_kind, self.max_members)
        self.calls, self.seeds_seen = [], []
        self._state = None
        self.scale, self.bank, self.evals = None, np.zeros((0, self.P), np.float32), []          # DenseGaHostEngine's
        self.dim, self._arch, self._last_n, self.g = 4, np.zeros((0, 4), np.float32), 0, None    # DenseNoveltyHostEngine's
        self.novelties = []                                                                     # DenseGaNsHostEngine's


def host_engine(hidden=(), nonlin="relu", max_members=16):
    e = AcrobotHostEngine(hidden, nonlin, max_members)
    e.noise_upload(D.noise())
    return e


def device_engine(hidden=(), nonlin="relu", max_members=16):
    """a live KIND_DENSE handle on the acrobot, the table uploaded"""
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_DENSE, ACT, max_members=max_members, env=_lib.ENV_ACROBOT, hidden=hidden, nonlin=nonlin)
    e.noise_upload(D.noise())
    return e


def base_thetas(hidden):
    """two base vectors (slots 0 and 1), as dense_support.base_thetas forms them: noise * scale_by at two offsets, the second three times as wide"""
    from dne_hip import policies
    P = num_params(hidden)
    sb = policies.dense_scale_by(ENV, hidden, ACT)
    tab = D.noise()
    return np.stack([tab[1234:1234 + P] * sb, tab[55555:55555 + P] * sb * np.float32(3.0)]).astype(np.float32)


def es_exp(model="LinearClassifier", **over):
    e = D.exp(GAME, model=model, episode_cutoff_mode=60, population_size=16)
    e.update(over)
    return e


def ga_exp(model="LinearClassifier", **over):
    e = {"game": GAME, "model": model, "population_size": 16, "selection_threshold": 4, "validation_threshold": 2, "num_validation_episodes": 2,
         "num_test_episodes": 2, "timesteps": 10 ** 9, "episode_cutoff_mode": 60, "mutation_power": 0.02}
    e.update(over)
    return e


def ns_exp(algo_type="ns", model="LinearClassifier", **over):
    e = {"game": GAME, "model": model, "algo_type": algo_type, "population_size": 16, "timesteps": 10 ** 9,
         "novelty_search": {"k": 2, "population_size": 3, "num_rollouts": 1, "selection_method": "round_robin"},
         "episode_cutoff_mode": 60, "return_proc_mode": "centered_sign_rank", "l2coeff": 0.005, "mutation_power": 0.02,
         "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}}
    e.update(over)
    return e
