"""TEST-ONLY support for the dense kind (csrc/dense.h, DNE_KIND_DENSE, dne_stepenv_act / _run): the shapes both test files
run, the members they set, the numpy restatement of the forward pass (maze_support.fmaf32: a correctly rounded fmaf, so no second implementation
of it), and DenseHostEngine -- _lib.Engine's surface for this kind over the CPU twins (dne_dense_forward_host / _rollout_host and
StepEnvHostEngine), with the update of update_support's numpy lines, so that envs and the drivers run without a GPU.  tests/test_dense_cpu.py
runs on it, tests/test_gpu_dense.py compares a live handle with it.  Every comparison is bit for bit (stepenv_support.same)."""
import numpy as np

import maze_support as MS
import pendulum_support as PS
import stepenv_support as SS
import update_support as U
from stepenv_support import same   # noqa: F401 (re-exported)

# the smallest shapes at which indexing can go wrong: no hidden layer, one unit, the baked (16, 16), unequal odd widths, the LDS maximum, tanh
SHAPES = (((), "relu"), ((1,), "relu"), ((16, 16), "relu"), ((5, 33), "relu"), ((64, 64, 64), "relu"), ((64,), "tanh"))
PENDULUM_SHAPES = (((), "relu"), ((5, 33), "relu"), ((64,), "tanh"))
CASES = tuple((env, h, nl) for env in ("maze", "cartpole") for h, nl in SHAPES) + tuple(("pendulum", h, nl) for h, nl in PENDULUM_SHAPES)
N_OUT = {"maze": 2, "cartpole": 2, "pendulum": 1}
N_IN = {"maze": 11, "cartpole": 4, "pendulum": 3}
SIGMA = 0.05

REFUSED = {
    "kind": "needs a DNE_KIND_DENSE engine",
    "members": "no members set",
    "member": r"member -?\d+ at position \d+ is out of range",
    "max_steps": "at least one act -> step round is needed",
}


def case_id(case):
    env, hidden, nl = case
    return "%s-%s-%s" % (env, "x".join(str(w) for w in hidden) or "linear", nl)


def dims_of(env, hidden):
    return (N_IN[env],) + tuple(hidden) + (N_OUT[env],)


def num_params(env, hidden):
    d = dims_of(env, hidden)
    return sum((d[l] + 1) * d[l + 1] for l in range(len(d) - 1))


def noise():
    return MS.maze_noise()


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------------------
def fmaf32(a, b, c):
    """maze_support.fmaf32, and where the sum leaves float32's range the infinity it rounds to: there the helper's tie test compares
    inf - s with inf - FLT_MAX, both infinite, and would step back to FLT_MAX (its callers never come near the range's end; 1e30 parameters do)"""
    r = MS.fmaf32(a, b, c)
    with np.errstate(all="ignore"):
        s = (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64) + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)
    return np.where(np.isinf(s), s, r).astype(np.float32)


def forward_np(env, hidden, nonlin, theta, obs):
    """theta [n][P], obs [n][IN] -> (the hidden layers behind their nonlinearity, concatenated [n][sum(hidden)]; out [n][OUT]): per unit one
    fmaf chain over k ascending from +0.0f, then + b, then the nonlinearity; none behind the last layer"""
    theta, x = np.asarray(theta, np.float32), np.asarray(obs, np.float32)
    d = dims_of(env, hidden)
    n, o, layers = theta.shape[0], 0, []
    for l in range(len(d) - 1):
        w = theta[:, o:o + d[l] * d[l + 1]].reshape(n, d[l], d[l + 1]); o += d[l] * d[l + 1]
        b = theta[:, o:o + d[l + 1]]; o += d[l + 1]
        acc = np.zeros((n, d[l + 1]), np.float32)
        with np.errstate(all="ignore"):
            for k in range(d[l]):
                acc = fmaf32(np.repeat(x[:, k:k + 1], d[l + 1], axis=1), w[:, k, :], acc)
            v = (acc + b).astype(np.float32)
        if l < len(d) - 2:
            x = PS.tanh_header(v).reshape(v.shape) if nonlin == "tanh" else np.where(v > 0, v, np.float32(0.0)).astype(np.float32)
            layers.append(x)
        else:
            x = v
    return (np.concatenate(layers, axis=1) if layers else np.zeros((n, 0), np.float32)), x


def action_np(env, out):
    """what the environment's step takes: the maze the two raw outputs, the cart-pole the first maximum (a tie or a NaN: 0), the pendulum the raw output"""
    if env == "maze":
        return np.ascontiguousarray(out, np.float32)
    if env == "cartpole":
        return (out[:, 1] > out[:, 0]).astype(np.int32)
    return np.ascontiguousarray(out[:, 0], np.float32)


# ---- thetas and members ------------------------------------------------------------------------------------------------------------------------
def base_thetas(env, hidden):
    """two base vectors (slots 0 and 1): TrainingState.initialize's noise * scale_by at two offsets, the second one three times as wide"""
    from dne_hip import policies
    P = num_params(env, hidden)
    sb = policies.dense_scale_by(SS.kind_id(env), hidden, N_OUT[env])
    tab = noise()
    b0 = tab[1234:1234 + P] * sb
    b1 = tab[55555:55555 + P] * sb * np.float32(3.0)
    if env == "pendulum":   # (a torque that leaves [-2, 2] now and then)
        b1 = b1 * np.float32(20.0)
    return np.stack([b0, b1]).astype(np.float32)


def member_table(env, hidden):
    """(slot, off, scale) of 7 members: base slots 0 and 1, scales +sigma, -sigma and 0, one offset at the table's last admissible position"""
    P = num_params(env, hidden)
    last = noise().size - P
    slot = np.array([0, 0, 1, 1, 0, 1, 0], np.int32)
    off = np.array([100, 100, 7777, last, 31, 0, last], np.int64)
    scale = np.array([SIGMA, -SIGMA, SIGMA, -SIGMA, 0.0, 0.0, 1.0], np.float32)
    return slot, off, scale


def member_thetas(env, hidden, bases=None, table=None):
    """the members' vectors: base[slot] + fl(scale * noise[off + p]), two roundings"""
    bases = base_thetas(env, hidden) if bases is None else bases
    slot, off, scale = member_table(env, hidden) if table is None else table
    tab, P = noise(), bases.shape[1]
    return np.stack([(bases[s] + np.float32(c) * tab[o:o + P]).astype(np.float32) for s, o, c in zip(slot, off, scale)])


def knife_thetas(env, hidden):
    """cart-pole members on the argmax's edge: all zeros (two equal logits: action 0), then the two logits one ulp apart either way (every
    weight 0, so each hidden layer is nonlin(0) = 0 and the outputs are the last biases)"""
    P = num_params(env, hidden)
    th = np.zeros((3, P), np.float32)
    one, up = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    th[1, -2:] = (one, up)     # out1 > out0 by one ulp: action 1
    th[2, -2:] = (up, one)     # out0 > out1 by one ulp: action 0
    return th


def spread_seeds(case, thetas, n=5, want=3):
    """n cart-pole seeds under which thetas[:n] end at `want` or more different steps (the twin says so), searched in a fixed order"""
    from dne_hip import _lib
    env, hidden, nl = case
    pool = SS.mixed_seeds(64)
    for k in range(0, 64 - n):
        seeds = pool[k:k + n]
        ln = _lib.dense_rollout_host(thetas[:n], SS.kind_id(env), hidden, nl, N_OUT[env], seeds=seeds)["lengths"]
        if len(set(ln.tolist())) >= want:
            return seeds
    raise AssertionError("no window of the seed pool spreads the episode lengths")


# ---- the CPU twins behind the Engine surface ----------------------------------------------------------------------------------------------------
class DenseHostEngine:
    """The dense kind without a GPU.  Evaluations are dne_dense_rollout_host on thetas perturbed in numpy; the environments are a
    StepEnvHostEngine of the shape's environment; stepenv_act is dne_dense_forward_host on the batch's observations and stepenv_run a loop of
    it and the host step; the update is update_support's numpy lines (the ones tests/test_gpu_update.py holds the kernels to bit for bit)."""

    def __init__(self, env, hidden=(), nonlin="relu", max_members=16, **kw):
        from dne_hip import _lib
        self.env = env
        self.kind, self.env_kind = _lib.KIND_DENSE, SS.kind_id(env)
        self.hidden, self.nonlin_name, self.nonlin = tuple(int(w) for w in hidden), nonlin, _lib.DENSE_NONLINS[nonlin]
        self.n_actions, self.max_members, self.ref_count = N_OUT[env], int(max_members), 0
        self.P = _lib.dense_num_params(self.env_kind, self.hidden, self.n_actions)
        assert self.P == num_params(env, self.hidden)
        self.bc_max_steps, self.bc_final_only = 0, False
        self.slots = {0: np.zeros(self.P, np.float32)}
        self.noise = self.members = None
        self.m, self.v, self.t = np.zeros(self.P, np.float32), np.zeros(self.P, np.float32), 0
        self.envs = SS.StepEnvHostEngine(self.env_kind, self.max_members)
        self.calls, self.seeds_seen = [], []
        self._state = None

    def close(self):
        pass

    def check_redzones(self):
        return 0

    # ---- parameters, noise, members
    def noise_upload(self, noise):
        self.noise = np.ascontiguousarray(noise, np.float32)

    def set_theta(self, theta, slot=0):
        theta = np.array(theta, np.float32).reshape(-1)
        assert theta.size == self.P
        self.slots[int(slot)] = theta

    def get_theta(self, slot=0):
        return self.slots[int(slot)].copy()

    def set_members(self, slot, off, scale):
        self.members = (np.asarray(slot, np.int32).copy(), np.asarray(off, np.int64).copy(), np.asarray(scale, np.float32).copy())

    def _theta_of(self, slot, off, scale):
        return (self.slots[int(slot)] + np.float32(scale) * self.noise[int(off):int(off) + self.P]).astype(np.float32)

    def member_thetas(self, which):
        slot, off, scale = self.members
        return np.stack([self._theta_of(slot[i], off[i], scale[i]) for i in which])

    def maze_set_walls(self, header, lines):
        from dne_hip import _lib
        if self.env_kind != _lib.KIND_MAZE:
            raise _lib.DneError("dne_maze_set_walls needs a DNE_KIND_MAZE engine (this one: kind %d)" % self.kind)
        self.envs.maze_set_walls(header, lines)

    # ---- whole episodes
    def _run(self, thetas, tslimit, seeds):
        from dne_hip import _lib
        seeds = np.asarray(seeds, np.uint32).reshape(-1)[:len(thetas)]
        self.seeds_seen.append(seeds.copy())
        if int(tslimit) <= 0:
            raise _lib.DneError("timestep limit must be positive")
        r = _lib.dense_rollout_host(np.stack(thetas), self.env_kind, self.hidden, self.nonlin, self.n_actions, seeds=seeds, tslimit=int(tslimit),
                                    **self.envs._maze())
        self._state = r["state"]
        return r["returns"], r["signreturns"], r["lengths"]

    def es_eval(self, idx, sigma, tslimit, seeds, want_bc=False):
        idx = np.asarray(idx, np.int64)
        self.calls.append(("es_eval", len(idx)))
        self.set_members(np.zeros(2 * len(idx), np.int32), np.repeat(idx, 2), np.tile(np.array([sigma, -sigma], np.float32), len(idx)))
        ret, sg, ln = self._run(list(self.member_thetas(range(2 * len(idx)))), tslimit, seeds)
        return ret.reshape(-1, 2), sg.reshape(-1, 2), ln.reshape(-1, 2)

    def eval_members(self, n, tslimit, seeds, want_bc=False):
        from dne_hip import _lib
        if self.members is None or len(self.members[0]) < n:
            raise _lib.DneError("dne_eval_members: %d members asked for, dne_set_members set %d" % (n, 0 if self.members is None else len(self.members[0])))
        return self._run(list(self.member_thetas(range(n))), tslimit, seeds)

    def dense_final_state(self, n):
        return self._state[:n].copy()

    # ---- the environments, and the policy behind them
    def __getattr__(self, name):
        if name in ("stepenv_reset", "stepenv_step", "stepenv_observation", "stepenv_state", "stepenv_set_state"):
            return getattr(self.envs, name)
        raise AttributeError(name)

    def _policy_args(self, call, indices, members, n):
        from dne_hip import _lib
        idx = self.envs._check(call, indices, n, True)
        if self.members is None or len(self.members[0]) < 1:
            raise _lib.DneError("%s: no members set (dne_set_members comes before the policy)" % call)
        mem = idx if members is None else np.asarray(members, np.int64).reshape(-1)
        for i, m in enumerate(mem.tolist()):
            if m < 0 or m >= len(self.members[0]):
                raise _lib.DneError("%s: member %d at position %d is out of range, dne_set_members set members 0..%d" % (call, m, i, len(self.members[0]) - 1))
        return idx, self.member_thetas(mem.tolist())

    def stepenv_act(self, indices=None, members=None, n=None):
        from dne_hip import _lib
        idx, th = self._policy_args("dne_stepenv_act", indices, members, n)
        _, out, act = _lib.dense_forward_host(th, self.envs.obs[idx], self.env_kind, self.hidden, self.nonlin, self.n_actions)
        return out, act

    def stepenv_run(self, max_steps, indices=None, members=None, n=None):
        from dne_hip import _lib
        if int(max_steps) < 1:
            raise _lib.DneError("dne_stepenv_run: max_steps = %d, at least one act -> step round is needed" % int(max_steps))
        idx, th = self._policy_args("dne_stepenv_run", indices, members, n)
        total, steps = np.zeros(idx.size, np.float64), np.zeros(idx.size, np.int32)
        done = self.envs.done[idx].astype(bool)
        for _ in range(int(max_steps)):
            if done.all():
                break
            live = ~done
            _, _, act = _lib.dense_forward_host(th, self.envs.obs[idx], self.env_kind, self.hidden, self.nonlin, self.n_actions)
            rew, done = self.envs.stepenv_step(act, idx)               # (a done environment keeps every bit and earns 0)
            total += rew.astype(np.float64)
            steps += live
        return total.astype(np.float32), steps, done

    # ---- the update: update_support's numpy lines
    def optimizer_reset(self):
        self.m, self.v, self.t = np.zeros(self.P, np.float32), np.zeros(self.P, np.float32), 0

    def optimizer_get_state(self):
        return self.m.copy(), self.v.copy(), self.t

    def optimizer_set_state(self, m, v, t):
        self.m, self.v, self.t = np.array(m, np.float32), np.array(v, np.float32), int(t)

    def es_update(self, idx, returns_n2, signreturns_n2, proc_mode, opt_kind, l2coeff, stepsize, beta1_or_momentum=0.9, beta2=0.999, epsilon=1e-8):
        self.calls.append(("es_update", len(idx)))
        assert opt_kind == "adam"
        rets = np.asarray(returns_n2, np.float32).reshape(-1, 2)
        g = U.weighted_sum_np(self.noise, idx, U.pair_weights_np(U.proc_np(rets, np.asarray(signreturns_n2, np.float32).reshape(-1, 2), proc_mode)), self.P, rets.size)
        self.t += 1
        self.slots[0], self.m, self.v, ratio = U.adam_np(self.slots[0], self.m, self.v, g, self.t, l2coeff, stepsize, beta1_or_momentum, beta2, epsilon)
        return ratio


def host_engine(case, max_members=16):
    env, hidden, nl = case
    e = DenseHostEngine(env, hidden, nl, max_members)
    if env == "maze":
        e.maze_set_walls(*MS.fixture_maze())
    e.noise_upload(noise())
    return e


def device_engine(case, max_members=16):
    """a live handle of the shape, the fixture maze loaded, the table uploaded"""
    from dne_hip import _lib
    env, hidden, nl = case
    e = _lib.Engine(_lib.KIND_DENSE, N_OUT[env], max_members=max_members, env=SS.kind_id(env), hidden=hidden, nonlin=nl)
    if env == "maze":
        e.maze_set_walls(*MS.fixture_maze())
    e.noise_upload(noise())
    return e


def load_members(e, case, extra=None):
    """base slots 0 and 1 and member_table's members (then `extra` thetas as plain members of their own slots 2.. at scale 0) -> their thetas"""
    env, hidden, _ = case
    bases = base_thetas(env, hidden)
    e.set_theta(bases[0], 0); e.set_theta(bases[1], 1)
    slot, off, scale = member_table(env, hidden)
    th = member_thetas(env, hidden, bases, (slot, off, scale))
    if extra is not None:
        for k, t in enumerate(extra):
            e.set_theta(t, 2 + k)
        slot = np.concatenate([slot, 2 + np.arange(len(extra), dtype=np.int32)])
        off = np.concatenate([off, np.zeros(len(extra), np.int64)])
        scale = np.concatenate([scale, np.zeros(len(extra), np.float32)])
        th = np.concatenate([th, np.asarray(extra, np.float32)])
    e.set_members(slot, off, scale)
    return th


# ---- the ES loop written out (tests 6 of the CPU file and 5 of the GPU file) ----------------------------------------------------------------------
def exp(game, **over):
    e = {"game": game, "model": "LinearClassifier", "num_test_episodes": 2, "population_size": 10, "timesteps": 10 ** 9,
         "episode_cutoff_mode": "env_default", "return_proc_mode": "centered_rank", "l2coeff": 0.005, "mutation_power": 0.02,
         "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}}
    e.update(over)
    return e


def shared_noise():
    from dne_hip import es
    t = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    t.noise = noise()
    t._engines = []
    return t


def plain_loop(env, iters, seed=4, pop=10, sigma=0.02, hidden=(), nonlin="relu"):
    """es_gpu.main's arithmetic for a dense model written out: theta0 = noise[idx0 : idx0 + P] * dense_scale_by with idx0 the stream's first draw,
    the test episodes' seeds drawn, then per iteration pop / 2 indices, pop seeds, the episodes (the twin), centered ranks, the weighted sum
    over 2N, Adam on -g + l2 * theta, and the test episodes' seeds again.  Returns per iteration (theta, m, v, returns [N][2], lengths [N][2])."""
    from dne_hip import _lib, policies
    tab = noise()
    kind = SS.kind_id(env)
    P = num_params(env, hidden)
    rs = np.random.RandomState(seed)
    theta = tab[rs.randint(0, tab.size - P + 1):][:P] * policies.dense_scale_by(kind, hidden, N_OUT[env])
    maze = dict(zip(("header", "lines"), MS.fixture_maze())) if env == "maze" else {}
    rs.randint(0, 2 ** 32, size=2, dtype=np.uint64)                      # the two test episodes before the loop
    m, v, out = np.zeros(P, np.float32), np.zeros(P, np.float32), []
    for it in range(1, iters + 1):
        idx = np.array([rs.randint(0, tab.size - P + 1) for _ in range(pop // 2)], np.int64)
        seeds = rs.randint(0, 2 ** 32, size=pop, dtype=np.uint64).astype(np.uint32)
        th = np.stack([(theta + np.float32(s) * tab[i:i + P]).astype(np.float32) for i in idx for s in (sigma, -sigma)])
        r = _lib.dense_rollout_host(th, kind, hidden, nonlin, N_OUT[env], seeds=seeds, **maze)
        rets = r["returns"].reshape(-1, 2)
        g = U.weighted_sum_np(tab, idx, U.pair_weights_np(U.ranks_np(rets)), P, rets.size)
        theta, m, v, _ = U.adam_np(theta, m, v, g, it, 0.005, 0.01)
        rs.randint(0, 2 ** 32, size=2, dtype=np.uint64)                  # the two test episodes after the update
        out.append((theta, m, v, rets, r["lengths"].reshape(-1, 2)))
    return out


TIMING_KEYS = ("TimestepsPerSecondThisIter", "TimeElapsedThisIter", "TimeElapsedThisIterTotal", "TimeElapsed", "TimeElapsedTotal")


def log_rows(log_dir):
    """the tabular rows es_gpu.main wrote into log.txt, one dict of strings per iteration, without the keys that hold wall-clock times"""
    import os
    rows, row = [], None
    for line in open(os.path.join(str(log_dir), "log.txt")):
        line = line.strip()
        if line.startswith("---"):
            if row:
                rows.append(row)
            row = {} if row is None or row else row
            continue
        if line.startswith("|") and row is not None:
            key, val = (p.strip() for p in line.strip("|").split("|"))
            if key not in TIMING_KEYS:
                row[key] = val
    return rows


def same_rows(a, b):
    """row by row: every value as printed, UpdateRatio to the print's six digits (the device adds the squares block by block, numpy pairwise:
    update_support.ratio_close)"""
    if len(a) != len(b):
        return False
    for ra, rb in zip(a, b):
        if ra.keys() != rb.keys():
            return False
        for k in ra:
            if k == "UpdateRatio":
                if abs(float(ra[k]) - float(rb[k])) > 2e-6 * abs(float(rb[k])):
                    return False
            elif ra[k] != rb[k]:
                return False
    return True
