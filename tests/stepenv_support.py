"""TEST-ONLY support for the step-at-a-time environments (csrc/step_env.h, dne_stepenv_*, dne_hip/envs.py): the scripted
action sequences, StepEnvHostEngine -- the stepenv_* surface of _lib.Engine over the host twins (dne_stepenv_reset_host / _step_host /
_observe_host: the same header compiled for the CPU), so that the Python classes run without a GPU -- the per-kind policies of the closed
loops (the host forward twins), and the checks both test files run: tests/test_stepenv_cpu.py on StepEnvHostEngine, tests/test_gpu_stepenv.py
on a live handle.  Every comparison is bit for bit."""
import numpy as np

import cartpole_support as CS
import maze_support as MS
import pendulum_support as PS

KINDS = ("maze", "cartpole", "pendulum")
GAMES = {"maze": "maze", "cartpole": "gym.CartPole-v1", "pendulum": "Pendulum-v0"}
OWN_LIMIT = {"maze": 400, "cartpole": 500, "pendulum": 200}
DIMS = {"maze": (11, 2, 7, False), "cartpole": (4, 1, 4, True), "pendulum": (3, 1, 2, False)}   # obs, act, state, int actions
PD_MEAN, PD_STD = np.array([0.1, -0.2, 0.3], np.float32), np.array([0.7, 0.6, 3.0], np.float32)   # test_gpu_pendulum.py's statistics

# what each refusal of the C ABI says (the engine's text and StepEnvHostEngine's)
REFUSED = {
    "kind": "needs a DNE_KIND_MAZE, DNE_KIND_CARTPOLE or DNE_KIND_PENDULUM engine",
    "n": r"environments asked for, the engine holds 1\.\.",
    "range": "is out of range",
    "twice": "is named twice",
    "never": "was never reset",
    "walls": "no maze loaded",
    "dtype": r"engine takes (int32|float) actions",
    "action": "CartPole-v1 has actions 0 and 1",
    "seeds": "seeds is NULL",
    "steps": "steps taken at position",
}


def kind_id(kind):
    from dne_hip import _lib
    return {"maze": _lib.KIND_MAZE, "cartpole": _lib.KIND_CARTPOLE, "pendulum": _lib.KIND_PENDULUM}[kind]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- scripted actions ----------------------------------------------------------------------------------------------------------------------------
def mixed_seeds(n):
    """n uint32 seeds that include 0, 2^31 and 2^32 - 1 as soon as there is room"""
    s = (np.arange(n, dtype=np.uint64) * 2654435761 + 12345) % (2 ** 32)
    for k, v in enumerate((0, 2 ** 31, 2 ** 32 - 1)):
        if k < n:
            s[k] = v
    return s.astype(np.uint32)


def scripted_actions(kind, n, T=None):
    """actions [T][n]...: the maze's from the reference recording's 32 sequences (member i plays sequence i mod 32), the cart-pole's random
    0 / 1 (so members end at different steps), the pendulum's uniform in [-3, 3] (so the torque clip works)"""
    T = OWN_LIMIT[kind] if T is None else T
    if kind == "maze":
        rec = np.load(MS.RECORDING)["actions"]
        return np.ascontiguousarray(np.stack([rec[i % rec.shape[0], :T] for i in range(n)], axis=1))
    rs = np.random.RandomState(4242 + n)
    if kind == "cartpole":
        return rs.randint(0, 2, (T, n)).astype(np.int32)
    return rs.uniform(-3, 3, (T, n)).astype(np.float32)


# ---- the host twins behind the Engine surface --------------------------------------------------------------------------------------------------
class StepEnvHostEngine:
    """max_members environments of one kind on the CPU: stepenv_reset / _step / _observation / _state / _set_state as _lib.Engine has them,
    each a gather of the named environments, one call of the host twin, and a scatter back; the refusals of the C ABI in its words."""

    def __init__(self, kind, max_members=8, **kw):
        from dne_hip import _lib
        self.kind = kind_id(kind) if isinstance(kind, str) else int(kind)
        self.max_members = int(max_members)
        self.obs_w, self.act_w, self.S, self.int_act = _lib.stepenv_dims(self.kind)
        self.header = self.lines = None
        M = self.max_members
        self.state, self.steps, self.limit = np.zeros((M, self.S), np.float64), np.zeros(M, np.int32), np.zeros(M, np.int32)
        self.done, self.obs, self.was_reset = np.zeros(M, np.uint8), np.zeros((M, self.obs_w), np.float32), np.zeros(M, bool)

    def close(self):
        pass

    def maze_set_walls(self, header, lines):
        self.header, self.lines = np.array(header, np.float32), np.array(lines, np.float32)

    def _maze(self):
        return dict(header=self.header, lines=self.lines)

    def _check(self, call, indices, n, reads):
        from dne_hip import _lib
        if self.kind == _lib.KIND_MAZE and self.header is None:
            raise _lib.DneError("%s: no maze loaded (dne_maze_set_walls comes before the environments)" % call)
        idx = np.arange(self.max_members if n is None else n, dtype=np.int64) if indices is None else np.asarray(indices, np.int64).reshape(-1)
        if idx.size < 1 or idx.size > self.max_members:
            raise _lib.DneError("%s: %d environments asked for, the engine holds 1..%d" % (call, idx.size, self.max_members))
        seen = set()
        for i, e in enumerate(idx.tolist()):
            if e < 0 or e >= self.max_members:
                raise _lib.DneError("%s: index %d at position %d is out of range, the engine holds environments 0..%d" % (call, e, i, self.max_members - 1))
            if e in seen:
                raise _lib.DneError("%s: environment %d is named twice" % (call, e))
            seen.add(e)
        if reads:
            for e in idx.tolist():
                if not self.was_reset[e]:
                    raise _lib.DneError("%s: environment %d was never reset (dne_stepenv_reset or dne_stepenv_set_state comes first)" % (call, e))
        return idx

    def _limit(self, max_steps):
        own = {7: 400, 4: 500, 2: 200}[self.S]
        return own if max_steps <= 0 or max_steps > own else int(max_steps)

    def stepenv_reset(self, indices=None, seeds=None, max_steps=0, n=None):
        from dne_hip import _lib
        idx = self._check("dne_stepenv_reset", indices, n, False)
        if self.kind != _lib.KIND_MAZE and seeds is None:
            raise _lib.DneError("dne_stepenv_reset: an engine of this kind resets every environment from its seed, seeds is NULL")
        st, t, lim, dn, ob = _lib.stepenv_reset_host(self.kind, idx.size, seeds, max_steps, **self._maze())
        self.state[idx], self.steps[idx], self.limit[idx], self.done[idx], self.obs[idx] = st, t, lim, dn, ob
        self.was_reset[idx] = True

    def stepenv_step(self, actions, indices=None, as_int=None):
        from dne_hip import _lib
        a = np.asarray(actions)
        idx = self._check("dne_stepenv_step", indices, a.shape[0] if a.ndim else 1, True)
        if as_int is not None and bool(as_int) != self.int_act:
            raise _lib.DneError("dne_stepenv_step: this engine takes %s actions" % ("int32" if self.int_act else "float"))
        st, t, lim, dn, ob = (np.ascontiguousarray(x[idx]) for x in (self.state, self.steps, self.limit, self.done, self.obs))
        rew = _lib.stepenv_step_host(self.kind, a, st, t, lim, dn, ob, **self._maze())
        self.state[idx], self.steps[idx], self.done[idx], self.obs[idx] = st, t, dn, ob
        return rew, dn.astype(bool)

    def stepenv_observation(self, indices=None, n=None):
        return self.obs[self._check("dne_stepenv_observation", indices, n, True)].copy()

    def stepenv_state(self, indices=None, n=None):
        idx = self._check("dne_stepenv_get_state", indices, n, True)
        return self.state[idx].copy(), self.steps[idx].copy(), self.done[idx].astype(bool)

    def stepenv_set_state(self, state, steps=None, indices=None, max_steps=0):
        from dne_hip import _lib
        state = np.ascontiguousarray(state, np.float64).reshape(-1, self.S)
        idx = self._check("dne_stepenv_set_state", indices, state.shape[0], False)
        steps = np.zeros(idx.size, np.int32) if steps is None else np.asarray(steps, np.int32).reshape(-1)
        lim = self._limit(max_steps)
        for i, t in enumerate(steps.tolist()):
            if t < 0 or t >= lim:
                raise _lib.DneError("dne_stepenv_set_state: %d steps taken at position %d, an environment under a limit of %d has taken 0..%d" % (t, i, lim, lim - 1))
        if self.S == 7:   # the maze keeps floats and ints: what the device stores is the state rounded to those types
            state = state.copy()
            state[:, :5] = state[:, :5].astype(np.float32).astype(np.float64)
        self.obs[idx] = _lib.stepenv_observe_host(self.kind, state, **self._maze())
        self.state[idx], self.steps[idx], self.limit[idx], self.done[idx] = state, steps, lim, 0
        self.was_reset[idx] = True


def host_engine(kind, max_members=8):
    e = StepEnvHostEngine(kind, max_members)
    if kind == "maze":
        e.maze_set_walls(*MS.fixture_maze())
    return e


def device_engine(kind, max_members=8, **kw):
    """a live handle of the kind, the fixture maze loaded"""
    from dne_hip import _lib
    if kind == "maze":
        e = _lib.Engine(_lib.KIND_MAZE, 2, max_members=max_members)
        e.maze_set_walls(*MS.fixture_maze())
    elif kind == "cartpole":
        e = _lib.Engine(_lib.KIND_CARTPOLE, 2, max_members=max_members)
    else:
        e = _lib.Engine(_lib.KIND_PENDULUM, 1, max_members=max_members, hidden=kw.get("hidden", 64), nonlin=kw.get("nonlin", "tanh"))
    return e


# ---- the policies of the closed loops: the host forward twins ------------------------------------------------------------------------------------
def policy(kind, thetas, hidden=64, nonlin="tanh"):
    """act(obs [n][obs]) -> actions for n environments, member i under thetas[i]"""
    from dne_hip import _lib
    thetas = np.ascontiguousarray(thetas, np.float32)
    if kind == "maze":
        return lambda obs: _lib.maze_forward_host(thetas, obs)[2]
    if kind == "cartpole":
        def act(obs):
            out = _lib.cartpole_forward_host(thetas, obs)[2]
            return (out[:, 1] > out[:, 0]).astype(np.int32)          # cartpole.h: pick_action
        return act
    return lambda obs: _lib.pendulum_forward_host(thetas, obs, hidden, PD_MEAN, PD_STD, nonlin=nonlin)[4]


def rollout_host(kind, thetas, seeds, tslimit, hidden=64, nonlin="tanh"):
    """the whole-episode host twin: (returns, lengths, final state as the environment's final_state / state has it)"""
    from dne_hip import _lib
    if kind == "maze":
        ret, ln, xy = _lib.maze_rollout_host(thetas, *MS.fixture_maze(), tslimit=tslimit)
        return ret, ln, xy
    if kind == "cartpole":
        return _lib.cartpole_rollout_host(thetas, seeds, tslimit)
    r = _lib.pendulum_rollout_host(thetas, seeds, hidden, PD_MEAN, PD_STD, nonlin=nonlin, tslimit=tslimit)
    return r["returns"], r["lengths"], r["state"]


def final_of(kind, env):
    """what rollout_host's third value is compared with"""
    return env.final_state() if kind == "maze" else env.state()[0]


def closed_loop_thetas(kind, hidden=64):
    """5 thetas per kind.  Cart-pole: theta = 0 first (equal logits, action 0: over within 11 steps), the balancing theta second."""
    from dne_hip import policies
    noise = MS.maze_noise()
    if kind == "maze":
        base = MS.theta0(noise)
        return np.stack([base, MS.straight_into_wall_theta(), MS.spin_in_place_theta(), MS.perturbed(base, noise, 100, 0.02), MS.perturbed(base, noise, 7777, 1.0)])
    if kind == "cartpole":
        base = CS.theta0(noise)
        return np.stack([np.zeros(CS.P, np.float32), CS.balancing_theta(), base, CS.perturbed(base, noise, 100, 0.02), CS.perturbed(base, noise, 7777, 1.0)])
    base = policies.normc_flat(hidden, 1, 3)
    base[PS.offsets(hidden, 1)[4]:] *= np.float32(150.0)              # (test_gpu_pendulum.py: actions leave +-2 now and then)
    return np.stack([base, np.zeros_like(base)] + [PS.perturbed(base, noise, o, s) for o, s in ((100, 0.02), (7777, 1.0), (31, -1.0))])


# ---- checks both files run -------------------------------------------------------------------------------------------------------------------------
def snapshot(e, n):
    """everything the batch holds for environments 0 .. n - 1"""
    st, t, dn = e.stepenv_state(n=n)
    return st, t, dn, e.stepenv_observation(n=n)


def same_snapshot(a, b):
    return all(same(x, y) for x, y in zip(a, b))


def check_done_freezes(e, kind):
    """an environment that is done, stepped three more times: reward 0, done 1, state, steps and observation keep every bit"""
    n, T = 3, 4
    acts = scripted_actions(kind, n, 40)
    e.stepenv_reset(n=n, seeds=mixed_seeds(n), max_steps=T)
    for t in range(T):
        rew, done = e.stepenv_step(acts[t])
        assert done.all() if t == T - 1 else not done.any()               # (no reset state of the cart-pole is within four steps of a threshold)
        if kind != "pendulum":
            assert same(rew, np.full(n, 1.0 if kind == "cartpole" else 0.0, np.float32))
    before = snapshot(e, n)
    assert np.array_equal(before[1], np.full(n, T, np.int32))
    for t in range(T, T + 3):
        rew, done = e.stepenv_step(acts[t])
        assert same(rew, np.zeros(n, np.float32)) and done.all() and same_snapshot(snapshot(e, n), before)


def check_subsets(e, kind):
    """indices [4, 0, 2] of a batch of 6: the others keep every bit, outputs come in the list's order; a reset of [3] alone"""
    n = 6
    seeds = mixed_seeds(n)
    acts = scripted_actions(kind, n, 3)
    e.stepenv_reset(n=n, seeds=seeds)
    e.stepenv_step(acts[0])                                            # off the reset state
    before = snapshot(e, n)
    sub = np.array([4, 0, 2], np.int32)
    # the same three environments stepped alone on a second batch: what the subset call has to give, in its order
    ref = host_engine(kind, n)
    ref.stepenv_reset(n=n, seeds=seeds)
    ref.stepenv_step(acts[0])
    want_rew, want_done = ref.stepenv_step(acts[1][sub], sub)
    rew, done = e.stepenv_step(acts[1][sub], sub)
    after = snapshot(e, n)
    assert same(rew, want_rew) and np.array_equal(done, want_done)
    for k in (1, 3, 5):
        assert all(same(a[k], b[k]) for a, b in zip(after, before)), k
    for k in sub:
        assert not same(after[0][k], before[0][k]) and after[1][k] == 2
    assert same(e.stepenv_observation(sub), after[3][sub]) and same(e.stepenv_observation(sub), ref.stepenv_observation(sub))
    st, t, dn = e.stepenv_state(sub)
    assert same(st, after[0][sub]) and np.array_equal(t, [2, 2, 2])
    assert same(e.stepenv_observation(sub[::-1].copy()), after[3][sub[::-1]])
    e.stepenv_reset(np.array([3], np.int32), seeds=np.array([99], np.uint32), max_steps=7)
    again = snapshot(e, n)
    for k in (0, 1, 2, 4, 5):
        assert all(same(a[k], b[k]) for a, b in zip(again, after)), k
    assert again[1][3] == 0 and not again[2][3]
    fresh = host_engine(kind, 1)
    fresh.stepenv_reset(n=1, seeds=np.array([99], np.uint32))
    assert same(again[0][3], fresh.stepenv_state(n=1)[0][0]) and same(again[3][3], fresh.stepenv_observation(n=1)[0])


def check_set_state(e, kind):
    """states no reset gives"""
    import math
    if kind == "cartpole":
        cases = CS.threshold_states()
        for a in (0, 1):
            e.stepenv_set_state(np.array([c[0] for c in cases]))
            st0, t0, dn0 = e.stepenv_state(n=len(cases))
            assert not dn0.any() and np.all(t0 == 0)
            assert same(e.stepenv_observation(n=len(cases)), st0.astype(np.float32))
            rew, done = e.stepenv_step(np.full(len(cases), a, np.int32))
            assert np.array_equal(done, np.array([c[1] for c in cases])) and same(rew, np.ones(len(cases), np.float32))
            st = e.stepenv_state(n=len(cases))[0]
            assert same(st[:, 0], st0[:, 0]) and same(st[:, 2], st0[:, 2])   # x + 0.02 * 0, theta + 0.02 * 0
    elif kind == "pendulum":
        e.stepenv_set_state(np.array([[math.pi / 2, 7.9], [0.0, 0.0]]))
        rew, done = e.stepenv_step(np.array([2.0, 0.0], np.float32))
        st = e.stepenv_state(n=2)[0]
        assert st[0, 1] == 8.0 and not done.any()                         # 7.9 + (15 sin(pi/2) + 6) * 0.05 = 8.95: clamped
        assert st[0, 0] == math.pi / 2 + (7.9 + (15.0 * PS.sincos_header(PS.norm_py(math.pi / 2))[0] + 3.0 * 2.0) * 0.05) * 0.05
        assert rew[1] == 0 and same(st[1], np.zeros(2))
        for _ in range(5):                                                   # from (0, 0) under 0 every reward is exactly 0
            rew, _ = e.stepenv_step(np.array([0.0], np.float32), np.array([1], np.int32))
            assert rew[0] == 0
        assert same(e.stepenv_state(np.array([1], np.int32))[0][0], np.zeros(2))
    else:
        hdr, _ = MS.fixture_maze()
        # 397 steps taken somewhere else: the third step from here is the 400th and pays -(distance to the goal); under max_steps 399 nothing is paid
        st = np.array([[float(hdr[2]) + 5.0, float(hdr[3]) - 3.0, 45.0, 1.0, -0.5, 0.0, 2.0]] * 2)
        e.stepenv_set_state(st[:1], steps=[397], indices=np.array([0], np.int32))
        e.stepenv_set_state(st[1:], steps=[397], indices=np.array([1], np.int32), max_steps=399)
        s0, t0, d0 = e.stepenv_state(n=2)
        assert same(s0, st) and np.array_equal(t0, [397, 397]) and not d0.any()
        rews, dones = [], []
        for _ in range(3):
            r, d = e.stepenv_step(np.zeros((2, 2), np.float32))
            rews.append(r); dones.append(d)
        s1 = e.stepenv_state(n=2)[0]
        assert np.array_equal(np.array(dones), [[False, False], [False, True], [True, True]])
        assert rews[0][0] == 0 and rews[1][0] == 0 and rews[2][0] < 0 and all(r[1] == 0 for r in rews)
        xy = s1[0, :2].astype(np.float32)
        d = np.sqrt((hdr[5] - xy[0]) * (hdr[5] - xy[0]) + (hdr[6] - xy[1]) * (hdr[6] - xy[1]), dtype=np.float32)
        assert same(rews[2][0], np.float32(-d))


def check_maze_limits(e):
    """max_steps 1, 399 and 400 (and 0 = 400, 5000 = 400) under one action sequence: done at the limit, the reward on step 400 alone"""
    limits = (1, 399, 400, 0, 5000)
    acts = scripted_actions("maze", 1)
    for k, lim in enumerate(limits):
        e.stepenv_reset(np.array([k], np.int32), max_steps=lim)
    idx = np.arange(len(limits), dtype=np.int32)
    total, first_done = np.zeros(len(limits)), np.zeros(len(limits), np.int32)
    for t in range(400):
        rew, done = e.stepenv_step(np.repeat(acts[t], len(limits), axis=0), idx)
        total += rew
        first_done[(first_done == 0) & done] = t + 1
        if t < 399:
            assert np.all(rew == 0)
    assert first_done.tolist() == [1, 399, 400, 400, 400]
    assert total[0] == 0 and total[1] == 0 and total[2] < 0 and total[2] == total[3] == total[4]
    st, steps, _ = e.stepenv_state(idx)
    assert steps.tolist() == [1, 399, 400, 400, 400]


def check_refusals(e, kind, fresh):
    """every refusal of the C ABI by name, the batch unchanged afterwards.  fresh(): a new engine of the kind on which nothing was reset (for the
    maze: no walls either)"""
    import pytest
    from dne_hip import _lib
    n = 4
    M = e.max_members
    seeds = mixed_seeds(n)
    e.stepenv_reset(n=n, seeds=seeds)
    e.stepenv_step(scripted_actions(kind, n, 1)[0])
    before = snapshot(e, n)
    act1 = scripted_actions(kind, 1, 1)[0]
    act2 = scripted_actions(kind, 2, 1)[0]

    def refused(what, fn):
        with pytest.raises(_lib.DneError, match=REFUSED[what]):
            fn()
        assert same_snapshot(snapshot(e, n), before), what

    refused("n", lambda: e.stepenv_reset(np.arange(M + 1, dtype=np.int32), seeds=np.zeros(M + 1, np.uint32)))
    refused("n", lambda: e.stepenv_observation(np.zeros(0, np.int32)))
    refused("range", lambda: e.stepenv_step(act1, np.array([M], np.int32)))
    refused("range", lambda: e.stepenv_step(act1, np.array([-1], np.int32)))
    refused("range", lambda: e.stepenv_reset(np.array([0, M], np.int32), seeds=seeds[:2]))
    refused("twice", lambda: e.stepenv_step(act2, np.array([1, 1], np.int32)))
    refused("twice", lambda: e.stepenv_reset(np.array([2, 2], np.int32), seeds=seeds[:2]))
    refused("twice", lambda: e.stepenv_set_state(before[0][:2], indices=np.array([0, 0], np.int32)))
    if M > n:
        refused("never", lambda: e.stepenv_step(act2, np.array([0, n], np.int32)))
        refused("never", lambda: e.stepenv_observation(np.array([n], np.int32)))
        refused("never", lambda: e.stepenv_state(np.array([n], np.int32)))
    refused("dtype", lambda: e.stepenv_step(np.zeros(2 if kind == "maze" else 1, np.float32 if kind == "cartpole" else np.int32), np.array([0], np.int32),
                                            as_int=kind != "cartpole"))
    refused("steps", lambda: e.stepenv_set_state(before[0][:1], steps=[OWN_LIMIT[kind]], indices=np.array([0], np.int32)))
    refused("steps", lambda: e.stepenv_set_state(before[0][:1], steps=[5], indices=np.array([0], np.int32), max_steps=5))
    if kind == "cartpole":
        refused("action", lambda: e.stepenv_step(np.array([0, 2, 1, 0], np.int32)))
        refused("action", lambda: e.stepenv_step(np.array([-1], np.int32), np.array([3], np.int32)))
    if kind != "maze":
        refused("seeds", lambda: e.stepenv_reset(n=n, seeds=None))
    f = fresh()
    try:
        with pytest.raises(_lib.DneError, match=REFUSED["walls" if kind == "maze" else "never"]):
            f.stepenv_step(act1, np.array([0], np.int32))
        with pytest.raises(_lib.DneError, match=REFUSED["walls" if kind == "maze" else "never"]):
            f.stepenv_observation(n=1)
        if kind == "maze":
            with pytest.raises(_lib.DneError, match=REFUSED["walls"]):
                f.stepenv_reset(n=1)
    finally:
        f.close()
