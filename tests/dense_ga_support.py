"""TEST-ONLY support for Deep-GA on the dense kind (csrc/dense_ga.h): maze_ga_support's contract in float32 numpy (IEEE,
unfused) with P a parameter, the shapes, genomes and descriptors both test files share, DenseGaHostEngine -- DenseHostEngine plus the
dense_ga_* surface from the two host twins (dne_dense_ga_theta_host / dne_dense_ga_members_host) and dne_dense_rollout_host, so that
ga_gpu.dense_main runs without a GPU -- and plain_loop: the same algorithm the reference's way, full lists, every theta rebuilt in numpy from
its WHOLE genome each generation.  Every comparison is bit for bit."""
import functools

import numpy as np

import dense_support as D
import maze_support as M
import stepenv_support as SS

# the smallest shapes at which kernels of 256-wide blocks with P at run time can go wrong
CASES = (("maze", (), "relu"),               # P = 24: one partly filled block
         ("pendulum", (51,), "tanh"),        # P = 256: exactly one full block, (3 + 1) * 51 + 52
         ("cartpole", (5, 33), "relu"),      # P = 291: one full block and a 35-wide tail
         ("maze", (16, 16), "relu"),         # P = 498: maze_ga.h's own case
         ("maze", (64, 64, 64), "relu"))     # P = 9218: 37 blocks, the last holding 2
PS = (24, 256, 291, 498, 9218)
CHAIN_LENGTHS = (1, 2, 9, 18)
POWERS = (0.0, 0.005, -0.02, 1e-30, 1e30)
BANKS = (0, 1, 3, 5)
COUNTS = (1, 3, 5, 9)
case_id = D.case_id


def num_params(case):
    return D.num_params(case[0], case[1])


@functools.lru_cache(maxsize=None)
def scale_by(case):
    from dne_hip import policies
    env, hidden, _ = case
    sb = np.asarray(policies.dense_scale_by(SS.kind_id(env), hidden, D.N_OUT[env]), np.float32)
    sb.setflags(write=False)
    return sb


@functools.lru_cache(maxsize=None)
def noise():
    n = M.maze_noise()
    n.setflags(write=False)
    return n


# ---- the contract in numpy, P = len(scale_by) -----------------------------------------------------------------------------------------------------
def perturbed(base, table, off, scale):
    """theta_p = base_p + fl(scale * noise[off + p]): two fp32 roundings"""
    base = np.asarray(base, np.float32)
    with np.errstate(all="ignore"):
        return (base + np.float32(scale) * table[off:off + base.size]).astype(np.float32)


def root_theta(table, sb, idx):
    return (table[idx:idx + sb.size] * sb).astype(np.float32)


def split(genome):
    root = genome[0]
    return int(root[0] if isinstance(root, (tuple, list)) else root), [(int(i), p) for i, p in genome[1:]]


def genome_theta(table, sb, genome):
    idx0, rest = split(genome)
    th = root_theta(table, sb, idx0)
    for idx, power in rest:
        th = perturbed(th, table, idx, power)
    return th


def member_theta(table, sb, bank, parent, idx, power):
    if parent < 0:
        return root_theta(table, sb, idx)
    if idx < 0:
        return np.array(bank[parent], np.float32)
    return perturbed(bank[parent], table, idx, power)


def members_theta(table, sb, bank, parent, idx, power):
    power = np.broadcast_to(np.asarray(power, np.float32), np.shape(parent))
    return np.stack([member_theta(table, sb, bank, int(a), int(b), c) for a, b, c in zip(parent, idx, power)])


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------------------
def make_genome(P, length, seed, count=None):
    """a genome of `length` seeds: indices from the whole table with 0 and count - P among them, powers cycling through POWERS"""
    rs = np.random.RandomState(500 + 17 * length + seed + P)
    last = (noise().size if count is None else count) - P
    idx = [int(v) for v in rs.randint(0, last + 1, size=length)]
    if length >= 2:
        idx[seed % length] = 0 if seed % 2 == 0 else last
    if length >= 9:
        idx[(seed + 3) % length] = last if seed % 2 == 0 else 0
    return (idx[0], ) + tuple((idx[j], POWERS[(j + seed) % len(POWERS)]) for j in range(1, length))


def genomes(P, count=None):
    """two genomes of every length in CHAIN_LENGTHS, and the two one-seed roots at the table's ends"""
    last = (noise().size if count is None else count) - P
    return [make_genome(P, n, s, count) for n in CHAIN_LENGTHS for s in (0, 1)] + [(0, ), (last, )]


def bank_genomes(P, T, count=None):
    """T parents of mixed depth (1, 9, 18, 2 seeds)"""
    return [make_genome(P, (1, 9, 18, 2, 9)[j % 5], 40 + j, count) for j in range(T)]


def descriptors(P, T, n, seed=0, kept=False, count=None):
    """n descriptors over a bank of T: roots, power-0 parents at idx 0, children at every power, the table's two ends among the indices; with
    `kept` the kept form too -- to another index than its own, and one source named twice"""
    rs = np.random.RandomState(900 + 31 * T + 7 * n + seed)
    last = (noise().size if count is None else count) - P
    parent, idx, power = [], [], []
    roots = children = 0
    for i in range(n):
        form = (i + seed) % (4 if kept else 3)
        if form == 0 or T == 0:
            parent.append(-1); idx.append((last, 0, int(rs.randint(0, last + 1)))[roots % 3]); power.append(POWERS[i % len(POWERS)])   # (a root's power is not read)
            roots += 1
        elif form == 1:
            parent.append(int(rs.randint(T))); idx.append(0); power.append(0.0)
        elif form == 2:
            parent.append((T - 1 - i) % T); idx.append((last, int(rs.randint(0, last + 1)), 0)[children % 3]); power.append(POWERS[(i + 1) % len(POWERS)])
            children += 1
        else:
            parent.append((i + 1) % T); idx.append(-1 - (i % 2) * 41); power.append(POWERS[i % len(POWERS)])
    if kept and n >= 2 and T >= 1:                                 # the same source twice, at other indices than its own when T allows
        parent[-2:], idx[-2:] = [n % T, n % T], [-7, -1]
    return np.array(parent, np.int32), np.array(idx, np.int64), np.array(power, np.float32)


def eval_descriptors(P, T, n, seed=0):
    """an evaluation's members over a bank of T: descriptors() without the kept form and without the powers no episode survives (1e30 makes
    every output infinite or NaN, which is its own test in the twins; here the episodes should differ)"""
    parent, idx, power = descriptors(P, T, n, seed)
    return parent, idx, np.where(np.abs(power) > 1.0, np.float32(0.05), power).astype(np.float32)


def signed_zero_noise(P):
    """a table whose first 2 P entries give a root every bias of which is -0.0 (scale_by is 0 there: the zero carries the noise's sign)"""
    n = noise().copy()
    n[:P] = -np.abs(n[:P])
    n[P:2 * P] = np.abs(n[P:2 * P])
    n.setflags(write=False)
    return n


def bias_positions(case):
    return np.flatnonzero(scale_by(case) == 0)


# ---- the dense_ga_* surface without a GPU --------------------------------------------------------------------------------------------------------------
class DenseGaHostEngine(D.DenseHostEngine):
    """DenseHostEngine plus what ga_gpu.dense_main asks of a KIND_DENSE engine: the bank as a numpy array filled by the two host twins, episodes
    through dne_dense_rollout_host.  Every dense_ga_* call is recorded in self.calls; every evaluation in self.evals (parent, idx, returns,
    lengths, seeds)."""

    def __init__(self, env, hidden=(), nonlin="relu", max_members=16, **kw):
        super().__init__(env, hidden, nonlin, max_members, **kw)
        self.scale = None
        self.bank = np.zeros((0, self.P), np.float32)
        self.evals = []

    def ga_select(self, returns, t):
        import oracle as O
        return O.ga_select(returns, t)

    def _need(self, call, walls=False):
        from dne_hip import _lib
        if self.scale is None:
            raise _lib.DneError("%s: no init scale" % call)
        if self.noise is None:
            raise _lib.DneError("%s: noise table not uploaded" % call)
        if walls and self.env_kind == _lib.KIND_MAZE and self.envs.header is None:
            raise _lib.DneError("%s: no maze loaded" % call)

    def _count(self, call, n):
        from dne_hip import _lib
        if not 1 <= n <= self.max_members:
            raise _lib.DneError("%s: %d outside [1, max_members = %d]" % (call, n, self.max_members))

    def dense_ga_set_init_scale(self, sb):
        self.calls.append(("dense_ga_set_init_scale", ))
        self.scale = np.array(sb, np.float32)
        assert self.scale.size == self.P

    def dense_ga_build(self, genomes):
        from dne_hip import _lib
        self._need("dense_ga_build")
        self.calls.append(("dense_ga_build", len(genomes)))
        self._count("dense_ga_build", len(genomes))
        self.bank = np.stack([_lib.dense_ga_theta_host(self.noise, self.scale, g) for g in genomes])

    def dense_ga_eval(self, parent, idx, power, tslimit, env_seed=None):
        from dne_hip import _lib
        self._need("dense_ga_eval", walls=True)
        parent, idx = np.asarray(parent, np.int32).reshape(-1), np.asarray(idx, np.int64).reshape(-1)
        self.calls.append(("dense_ga_eval", len(parent)))
        self._count("dense_ga_eval", len(parent))
        if np.any(idx < 0):
            raise _lib.DneError("dense_ga_eval: the kept form is for promotion only")
        if self.env_kind != _lib.KIND_MAZE and env_seed is None:
            raise _lib.DneError("dense_ga_eval: env_seed is NULL")
        th = _lib.dense_ga_members_host(self.noise, self.scale, self.bank if len(self.bank) else None, parent, idx, power)
        seeds = np.zeros(len(parent), np.uint32) if env_seed is None else np.asarray(env_seed, np.uint32)
        out = self._run(list(th), tslimit, seeds)
        self.evals.append((parent.copy(), idx.copy(), out[0].copy(), out[2].copy(), None if env_seed is None else seeds.copy()))
        return out

    def dense_ga_promote(self, parent, idx, power):
        from dne_hip import _lib
        self._need("dense_ga_promote")
        parent = np.asarray(parent, np.int32).reshape(-1)
        self.calls.append(("dense_ga_promote", len(parent)))
        self._count("dense_ga_promote", len(parent))
        self.bank = _lib.dense_ga_members_host(self.noise, self.scale, self.bank if len(self.bank) else None, parent, idx, power)

    def dense_ga_parents(self):
        return len(self.bank)

    def dense_ga_get_parent(self, j):
        return self.bank[j].copy()


def host_engine(case, max_members=16):
    env, hidden, nl = case
    e = DenseGaHostEngine(env, hidden, nl, max_members)
    if env == "maze":
        e.maze_set_walls(*M.fixture_maze())
    e.noise_upload(noise())
    return e


def device_engine(case, max_members=16):
    """a live handle of the shape: the fixture maze loaded, the table uploaded, the init scale set"""
    e = D.device_engine(case, max_members)
    e.dense_ga_set_init_scale(scale_by(case))
    return e


def rollout(case, thetas, tslimit, seeds=None):
    """dne_dense_rollout_host on thetas [n][P] (tslimit <= 0: the environment's own limit) -> dict(returns, signreturns, lengths, state)"""
    from dne_hip import _lib
    env, hidden, nl = case
    maze = dict(zip(("header", "lines"), M.fixture_maze())) if env == "maze" else {}
    return _lib.dense_rollout_host(np.asarray(thetas, np.float32), SS.kind_id(env), hidden, nl, D.N_OUT[env], seeds=seeds, tslimit=tslimit, **maze)


# ---- the loop the reference's way ------------------------------------------------------------------------------------------------------------------------
class Individual(object):
    def __init__(self, seeds, reward, length):
        self.seeds, self.reward, self.length = seeds, reward, length


def plain_loop(case, exp, seed, iters, population=None, max_members=10):
    """gpu_implementation/ga.py:157-271 with nothing lazy, on the numpy statement above: every offspring gets its genome, every theta --
    offspring, validated individual, parent -- is rebuilt from its WHOLE genome each generation, the population is the full sorted list.
    Shared with the driver by decision, not by code: the two whole-array draws per generation; on the cart-pole the seeds of every
    evaluation call (at most max_members members each) drawn after them; a previous elite's re-evaluation as theta + fl(0 * noise[0:P])
    while a bank exists; test episodes at the environment's own limit.  -> one record per generation."""
    env = case[0]
    table, sb, P = noise(), scale_by(case), num_params(case)
    n, T, V, k = exp["population_size"], exp["selection_threshold"], exp["validation_threshold"], exp["num_validation_episodes"]
    power, cutoff = exp["mutation_power"], exp["episode_cutoff_mode"]
    assert isinstance(cutoff, int) and not isinstance(power, dict)
    rs = np.random.RandomState(seed)

    def run(thetas, limit):
        rets, lens = [], []
        for s in range(0, len(thetas), max_members):
            part = thetas[s:s + max_members]
            seeds = None if env == "maze" else rs.randint(0, 2 ** 32, size=len(part), dtype=np.uint64).astype(np.uint32)
            r = rollout(case, np.stack(part), limit, seeds)
            rets.append(r["returns"]); lens.append(r["lengths"])
        return np.concatenate(rets), np.concatenate(lens)

    population = list(population or [])
    elite, best, best_val, best_test, timesteps = None, None, float("-inf"), float("-inf"), 0

    def next_parents():
        if not population or T <= 0:
            return []
        top = [o.seeds for o in population[:T]]
        if elite is None or elite.seeds in top:
            return top
        return [elite.seeds] + top[:T - 1]

    parents, records = next_parents(), []
    for _ in range(iters):
        if parents:
            of = rs.randint(len(parents), size=n)
        idx = rs.randint(0, table.size - P + 1, size=n)
        tasks = [tuple(parents[of[i]]) + ((int(idx[i]), power), ) if parents else (int(idx[i]), ) for i in range(n)]
        rets, lens = run([genome_theta(table, sb, g) for g in tasks], cutoff)
        results = [Individual(g, float(r), int(l)) for g, r, l in zip(tasks, rets, lens)]
        population = sorted(results, key=lambda o: o.reward, reverse=True)          # stable: equal rewards keep arrival order
        validated = population[:V]
        thetas = [genome_theta(table, sb, o.seeds) for o in validated]
        if elite is not None:
            validated = [elite] + validated[:-1]
            again = genome_theta(table, sb, elite.seeds)
            thetas = [perturbed(again, table, 0, 0.0) if parents else again] + thetas[:-1]
        vr, vl = run([th for th in thetas for _ in range(k)], cutoff)
        val = [float(np.mean(vr[i * k:(i + 1) * k])) for i in range(len(thetas))]
        elite_at = int(np.argmax(val))
        elite = validated[elite_at]
        er, _ = run([thetas[elite_at]] * exp["num_test_episodes"], 0)
        timesteps += int(np.sum(lens)) + int(np.sum(vl))
        if np.mean(val) > best_val:
            best, best_val, best_test = elite.seeds, float(np.mean(val)), float(np.mean(er))
        parents = next_parents()
        records.append(dict(parents=list(parents), thetas=[genome_theta(table, sb, g) for g in parents], elite=elite.seeds,
                            returns=np.array(rets, np.float32), top=[o.seeds for o in population[:max(T, V)]], curr_solution=best,
                            curr_solution_val=best_val, curr_solution_test=best_test, timesteps_so_far=timesteps))
    return records


def exp(game, model="LinearClassifier", **over):
    e = {"game": game, "model": model, "population_size": 10, "selection_threshold": 3, "validation_threshold": 2,
         "num_validation_episodes": 2, "num_test_episodes": 2, "episode_cutoff_mode": 40, "mutation_power": 0.005, "timesteps": 10 ** 9}
    if game == "maze":
        e["maze_file"] = M.MAZE_FILE
    e.update(over)
    return e


def shared_noise():
    return D.shared_noise()


log_rows = D.log_rows
