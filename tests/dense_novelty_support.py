"""TEST-ONLY support for novelty over final states on the dense kind (csrc/dense_novelty.h): the contract restated in
numpy float64, the point sets both test files share, DenseNoveltyHostEngine -- DenseHostEngine plus the archive, the BCs and dense_novelty
through the CPU twins, so that dne_hip/nses_gpu.py runs a dense policy without a GPU -- and that driver's loop written out (plain_loop: the
archive in numpy, novelty by the restatement).  Every comparison is bit for bit."""
import functools

import numpy as np

import dense_support as D
import maze_support as MS
import stepenv_support as SS
import update_support as U

KMAX, TILE = 32, 1024
DIMS = (2, 4)
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
COUNTS = (1, 2, 3, 4, 5, 9)                  # members: below, at and above the kernel's four per workgroup
KS = (1, 2, 25, 32, 40)                      # 40 > KMAX: the host takes it, the device refuses it
SETS = ("lattice", "random", "edge_few_nan", "edge_mostly_nan")
NAN, INF = np.float32("nan"), np.float32("inf")
BC_DIM = {"maze": 2, "cartpole": 4, "pendulum": 2}


# ---- the contract, restated in numpy float64 -----------------------------------------------------------------------------------------------------
def distances(p, archive):
    """float64 [narch]: d_i = a_i - p_i in double, s = d_0 * d_0, then s = s + d_i * d_i for i ascending, np.sqrt (correctly rounded)"""
    A, p = np.asarray(archive, np.float32).astype(np.float64), np.asarray(p, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d = A[:, 0] - p[0]
        s = d * d
        for i in range(1, A.shape[1]):
            d = A[:, i] - p[i]
            s = s + d * d
        return np.sqrt(s)


def order_of(dist):
    """the archive slots in the order (isnan, value, slot): a stable sort"""
    nan = np.isnan(dist)
    return np.lexsort((np.arange(dist.size), np.where(nan, 0.0, dist), nan))


def contract(bc, archive, k):
    archive = np.asarray(archive, np.float32)
    bc = np.asarray(bc, np.float32).reshape(-1, archive.shape[1])
    kk = min(int(k), archive.shape[0])
    out = np.empty(bc.shape[0], np.float64)
    for m, p in enumerate(bc):
        dist = distances(p, archive)
        total = 0.0
        with np.errstate(all="ignore"):
            for j in order_of(dist)[:kk]:
                total = total + dist[j]
            out[m] = total / kk
    return out


def same(a, b):
    return MS.same_nan(np.asarray(a, np.float64), np.asarray(b, np.float64))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the point sets ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def point_set(name, dim, narch):
    """(members float32 [9][dim], archive float32 [narch][dim]); the archives of one (name, dim) nest, except where the edge sets plant points"""
    rs = np.random.RandomState(100 * dim + SETS.index(name))
    if name == "lattice":       # integer coordinates in -3 .. 3: a handful of distinct distances, exact ties across slots, lanes and tiles
        return rs.randint(-3, 4, (9, dim)).astype(np.float32), rs.randint(-3, 4, (SIZES[-1], dim)).astype(np.float32)[:narch].copy()
    mem = rs.uniform(-10, 10, (9, dim)).astype(np.float32)
    arch = rs.uniform(-10, 10, (SIZES[-1], dim)).astype(np.float32)[:narch].copy()
    if name == "random":
        return mem, arch
    # the edge sets.  Members: its own point (planted in the archive twice), a NaN member, +inf, 1e30, +-0.0, 1e-40 (a float32 subnormal), -inf
    mem[1, 0] = NAN
    mem[2, 0] = INF
    mem[3] = np.float32(1e30)
    mem[4] = np.where(np.arange(dim) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    mem[5] = np.float32(1e-40)
    mem[6, dim - 1] = -INF
    plant = [mem[0], mem[0], -mem[4], np.full(dim, 1e30, np.float32), np.full(dim, -1e30, np.float32), np.full(dim, 1e-40, np.float32),
             np.where(np.arange(dim) == 0, INF, np.float32(1.0)), np.where(np.arange(dim) == dim - 1, -INF, np.float32(1.0))]
    slots = rs.permutation(narch)[:len(plant)] if narch >= 63 else np.arange(min(narch, 2))
    for s, q in zip(slots, plant):
        arch[s] = q
    if narch >= 63:
        free = np.setdiff1d(np.arange(narch), slots)
        if name == "edge_few_nan":          # 3 NaN points: fewer than kk at k >= 25, never reached
            nan_slots = free[rs.permutation(free.size)[:3]]
        else:                               # all but 5 of the free slots: more than narch - kk at k >= 25, the sum reaches them
            nan_slots = free[rs.permutation(free.size)[5:]]
        arch[nan_slots, rs.randint(0, dim, nan_slots.size)] = NAN
    return mem, arch


def grid(ks=KS):
    """every (set, dim, narch, n, k) of the issue's shapes"""
    for name in SETS:
        for dim in DIMS:
            for narch in SIZES:
                for n in COUNTS:
                    for k in ks:
                        yield name, dim, narch, n, k


@functools.lru_cache(maxsize=None)
def contract_of(name, dim, narch, k):
    """the restatement for all 9 members of a cell, computed once (members are scored independently: n members are its first n rows)"""
    mem, arch = point_set(name, dim, narch)
    return contract(mem, arch, k)


def tie_at_cut(name, dim, narch, ks=KS):
    """does some member of the cell have two archive points at equal distance on either side of position kk, for some k of the grid"""
    mem, arch = point_set(name, dim, narch)
    for p in mem:
        dist = distances(p, arch)
        srt = dist[order_of(dist)]
        for k in ks:
            if k < narch and srt[k - 1] == srt[k]:
                return True
    return False


# ---- the CPU twins behind the Engine surface -------------------------------------------------------------------------------------------------------
class DenseNoveltyHostEngine(D.DenseHostEngine):
    """DenseHostEngine plus what dne_hip/nses_gpu.py asks of a KIND_DENSE engine: the BCs of the last evaluation (dne_dense_bc_host), the
    archive, dense_novelty (dne_dense_novelty_host), and the three update calls of nses.blend_and_update in update_support's numpy lines."""

    def __init__(self, env, hidden=(), nonlin="relu", max_members=16, **kw):
        super().__init__(env, hidden, nonlin, max_members, **kw)
        self.dim = BC_DIM[env]
        self._arch = np.zeros((0, self.dim), np.float32)
        self._last_n, self.g = 0, None

    def _run(self, thetas, tslimit, seeds):
        out = super()._run(thetas, tslimit, seeds)
        self._last_n = len(thetas)
        return out

    def dense_bc_dim(self):
        return self.dim

    def _points(self, call, bc, n):
        from dne_hip import _lib
        if bc is not None:
            return np.asarray(bc, np.float32).reshape(-1, self.dim)
        n = self._last_n if n is None else int(n)
        if n < 1 or n > self._last_n:
            raise _lib.DneError("%s: %d members asked for, the last evaluation ran %d" % (call, n, self._last_n))
        return _lib.dense_bc_host(self.env_kind, self._state[:n])

    def dense_bc(self, n):
        return self._points("dne_dense_bc", None, n)

    def dense_archive_append(self, bc=None, n=None):
        self._arch = np.concatenate([self._arch, self._points("dne_dense_archive_append", bc, n)])

    def dense_archive_clear(self):
        self._arch = np.zeros((0, self.dim), np.float32)

    def dense_archive_size(self):
        return int(self._arch.shape[0])

    def dense_archive(self):
        return self._arch.copy()

    def dense_novelty(self, k, bc=None, n=None):
        from dne_hip import _lib
        if not 1 <= int(k) <= KMAX:
            raise _lib.DneError("dne_dense_novelty: k = %d outside 1..%d" % (k, KMAX))
        if not len(self._arch):
            raise _lib.DneError("dne_dense_novelty: the archive is empty")
        return _lib.dense_novelty_host(self._points("dne_dense_novelty", bc, n), self._arch, k, D=self.dim)

    # ---- nses.blend_and_update's three calls
    def centered_ranks(self, x):
        return U.ranks_np(np.asarray(x, np.float32))

    def weighted_sum(self, idx, w, denom, copy_out=True):
        self.g = U.weighted_sum_np(self.noise, idx, np.asarray(w, np.float32), self.P, denom)
        return self.g if copy_out else None

    def optimizer_step(self, kind, l2coeff, stepsize, beta1_or_momentum=0.9, beta2=0.999, epsilon=1e-8):
        assert kind == "adam"
        self.t += 1
        self.slots[0], self.m, self.v, ratio = U.adam_np(self.slots[0], self.m, self.v, self.g, self.t, l2coeff, stepsize, beta1_or_momentum, beta2, epsilon)
        return ratio


def host_engine(env, hidden=(), nonlin="relu", max_members=16):
    return DenseNoveltyHostEngine(env, hidden, nonlin, max_members)


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------------
GAMES = {"maze": "maze", "cartpole": "gym.CartPole-v1", "pendulum": "Pendulum-v0"}


def exp(env, **over):
    e = {"game": GAMES[env], "model": "LinearClassifier", "algo_type": "ns", "population_size": 8, "timesteps": 10 ** 9,
         "novelty_search": {"k": 2, "population_size": 3, "num_rollouts": 1, "selection_method": "round_robin"},
         "episode_cutoff_mode": "env_default", "return_proc_mode": "centered_sign_rank", "l2coeff": 0.005, "mutation_power": 0.02,
         "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}}
    if env == "maze":
        e["maze_file"] = MS.MAZE_FILE
    ns = dict(e["novelty_search"]); ns.update(over.pop("ns", {}))
    e.update(over); e["novelty_search"] = ns
    return e


def run(log_dir, iters, env="maze", eng=None, seed=4, **over):
    """nses_gpu.main on `eng` (default: a host engine without hidden layers) -> (state, engine)"""
    from dne_hip import nses_gpu
    eng = host_engine(env) if eng is None else eng
    return nses_gpu.main(str(log_dir), engine=eng, noise=D.shared_noise(), seed=seed, max_iters=iters, **exp(env, **over)), eng


def same_state(a, b):
    ok = len(a.thetas) == len(b.thetas) and a.parents == b.parents and a.curr_parent == b.curr_parent and a.it == b.it
    ok = ok and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a.thetas, b.thetas))
    ok = ok and all(np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1])) and x[2] == y[2]
                    for x, y in zip(a.optimizers, b.optimizers))
    ok = ok and a.archive.shape == b.archive.shape and np.array_equal(bits(a.archive), bits(b.archive)) and same(np.array(a.novelty_log), np.array(b.novelty_log))
    return bool(ok and a.timesteps_so_far == b.timesteps_so_far and all(np.array_equal(x, y) for x, y in zip(a.stream[1:], b.stream[1:])))


class Plain(object):
    """what plain_loop returns: the fields same_state reads"""


def plain_loop(env, iters, seed=4, hidden=(), nonlin="relu", **over):
    """nses_gpu.main's dense route written out on a bare DenseHostEngine (episodes and the numpy update only): the archive is a numpy array,
    the BCs are float32 casts of the final state records, novelty is contract()."""
    from dne_hip import _lib, policies
    cfg = exp(env, **over)
    ns = cfg["novelty_search"]
    M, k, R, method = ns["population_size"], ns["k"], ns["num_rollouts"], ns["selection_method"]
    n_pairs, sigma, mode, nsr = cfg["population_size"] // 2, np.float32(cfg["mutation_power"]), cfg["return_proc_mode"], cfg["algo_type"] == "nsr"
    dim, kind = BC_DIM[env], SS.kind_id(env)
    tab = D.noise()
    e = D.DenseHostEngine(env, hidden, nonlin, max(2 * n_pairs, M, 2))
    if env == "maze":
        e.maze_set_walls(*MS.fixture_maze())
    e.noise_upload(tab)
    P, own = e.P, {"maze": 400, "cartpole": 500}[env]
    rs = np.random.RandomState(seed)
    archive = np.zeros((0, dim), np.float32)
    bc_of = lambda n: e.dense_final_state(n)[:, :dim].astype(np.float32)

    def episodes(theta):
        """R episodes of theta at power 0 (pairs: (R + 1) // 2 of them, two seeds each) -> the archive point, the first return and length"""
        pairs = (R + 1) // 2
        seeds = rs.randint(0, 2 ** 32, size=2 * pairs, dtype=np.uint64).astype(np.uint32)
        e.set_theta(theta)
        ret, _, ln = e.es_eval(np.zeros(pairs, np.int64), 0.0, own, seeds)
        bc = bc_of(R)
        point = bc[0] if R == 1 else np.mean(bc.astype(np.float64), axis=0).astype(np.float32)
        return point, float(ret.reshape(-1)[0]), int(ln.reshape(-1)[0])

    thetas, opts = [], []
    for _ in range(M):
        theta = tab[rs.randint(0, tab.size - P + 1):][:P] * policies.dense_scale_by(kind, hidden, D.N_OUT[env])
        point, _, _ = episodes(theta)
        archive = np.concatenate([archive, point[None]])
        thetas.append(theta.astype(np.float32)); opts.append((np.zeros(P, np.float32), np.zeros(P, np.float32), 0))
    out = Plain()
    out.parents, out.novelty_log, out.it, out.timesteps_so_far, p = [], [], 0, 0, 0
    for _ in range(iters):
        theta, (m, v, t) = thetas[p], opts[p]
        idx = np.array([rs.randint(0, tab.size - P + 1) for _ in range(n_pairs)], np.int64)
        seeds = rs.randint(0, 2 ** 32, size=2 * n_pairs, dtype=np.uint64).astype(np.uint32)
        e.set_theta(theta)
        rets, _, lens = e.es_eval(idx, sigma, own, seeds)
        nov = contract(bc_of(2 * n_pairs), archive, k)
        nov = np.where(np.isfinite(nov), nov, 0.0)
        aux = nov.astype(np.float32).reshape(-1, 2)
        proc = U.ranks_np(rets) if mode == "centered_rank" else aux if mode == "sign" else U.ranks_np(aux)
        if nsr:
            proc = ((U.ranks_np(rets) + proc) / 2.0).astype(np.float32)
        g = U.weighted_sum_np(tab, idx, proc[:, 0] - proc[:, 1], P, float(rets.size))
        theta, m, v, _ = U.adam_np(theta, m, v, g, t + 1, 0.005, 0.01)
        point, _, _ = episodes(theta)
        archive = np.concatenate([archive, point[None]])
        thetas[p], opts[p] = theta, (m, v, t + 1)
        out.parents.append(p); out.novelty_log.append((float(nov.mean()), float(nov.max())))
        out.it += 1; out.timesteps_so_far += int(np.sum(lens))
        if method == "round_robin":
            p = (p + 1) % M
        else:
            sel = rs.randint(0, 2 ** 32, size=M, dtype=np.uint64).astype(np.uint32)
            r = _lib.dense_rollout_host(np.stack(thetas), kind, hidden, nonlin, D.N_OUT[env], seeds=sel, tslimit=own, **e.envs._maze())
            sn = contract(r["state"][:, :dim].astype(np.float32), archive, k)
            total = float(np.sum(sn))
            probs = sn / total if np.isfinite(total) and total > 0.0 and np.all(np.isfinite(sn)) else np.full(M, 1.0 / M)
            p = int(rs.choice(range(M), 1, p=probs)[0])
    out.thetas, out.optimizers, out.archive, out.curr_parent, out.stream = thetas, opts, archive, p, rs.get_state()
    return out
