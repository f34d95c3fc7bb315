"""TEST-ONLY support for Deep-GA on the hard maze (csrc/maze_ga.h): the contract in float32 numpy (IEEE, unfused), the
genomes and descriptors every test file shares, MazeGaHostEngine -- MazeHostEngine plus the maze_ga_* surface from that numpy statement and
dne_maze_rollout_host, so that dne_hip/ga_gpu.py's maze loop runs without a GPU -- and plain_loop: the same algorithm written the
reference's way, full Offspring lists and every parent rebuilt from its whole genome each generation."""
import functools

import numpy as np

import maze_support as M

P = M.P
CHAIN_LENGTHS = (1, 2, 8, 9, 10, 17, 18)        # seeds per genome: around k_chain_sum's 8-wide unroll with (n - 1 mutations) and without a root in front
POWERS = (0.0, 0.005, -0.02, 1e-30, 1e30)
BANKS = (1, 3, 5)
COUNTS = (1, 3, 4, 5, 9)                        # members: below, at and above k_maze_rollout's four per wave


def scale_by():
    from dne_hip import policies
    return policies.simple_scale_by()


# ---- the contract in numpy ----------------------------------------------------------------------------------------------------------------------
def root_theta(noise, idx):
    """fl(noise[idx + p] * scale_by[p])"""
    return (noise[idx:idx + P] * scale_by()).astype(np.float32)


def split(genome):
    """(idx0, (idx1, power1), ...) with the root as a bare index or a 1-tuple -> idx0, [(idx, power), ...]"""
    root = genome[0]
    return int(root[0] if isinstance(root, (tuple, list)) else root), [(int(i), p) for i, p in genome[1:]]


def genome_theta(noise, genome):
    """models/base.py:127-149: the root, then theta + fl(power * noise[idx:idx + P]) per mutation, in order (M.perturbed is that form)"""
    idx0, rest = split(genome)
    th = root_theta(noise, idx0)
    for idx, power in rest:
        th = M.perturbed(th, noise, idx, power)
    return th


def member_theta(noise, bank, parent, idx, power):
    """one descriptor: root (parent -1), kept (idx < 0: the parent's own bits), child"""
    if parent < 0:
        return root_theta(noise, idx)
    if idx < 0:
        return np.array(bank[parent], np.float32)
    return M.perturbed(bank[parent], noise, idx, power)


def members_theta(noise, bank, parent, idx, power):
    power = np.broadcast_to(np.asarray(power, np.float32), np.shape(parent))
    return np.stack([member_theta(noise, bank, int(a), int(b), c) for a, b, c in zip(parent, idx, power)])


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise():
    n = M.maze_noise()
    n.setflags(write=False)
    return n


def make_genome(length, seed):
    """a genome of `length` seeds: indices from the whole table with 0 and count - 498 among them, powers cycling through POWERS"""
    rs = np.random.RandomState(500 + 17 * length + seed)
    last = noise().size - P
    idx = [int(v) for v in rs.randint(0, last + 1, size=length)]
    if length >= 2:
        idx[seed % length] = 0 if seed % 2 == 0 else last
    if length >= 8:
        idx[(seed + 3) % length] = last if seed % 2 == 0 else 0
    return (idx[0], ) + tuple((idx[j], POWERS[(j + seed) % len(POWERS)]) for j in range(1, length))


@functools.lru_cache(maxsize=None)
def genomes():
    """two genomes of every length in CHAIN_LENGTHS, and the two one-seed roots at the table's ends"""
    out = [make_genome(n, s) for n in CHAIN_LENGTHS for s in (0, 1)]
    return tuple(out + [(0, ), (noise().size - P, )])


@functools.lru_cache(maxsize=None)
def genome_thetas():
    th = np.stack([genome_theta(noise(), g) for g in genomes()])
    th.setflags(write=False)
    return th


def bank_genomes(T):
    """T parents of mixed depth (1, 9, 18, 2, 10 seeds)"""
    return [make_genome((1, 9, 18, 2, 10)[j % 5], 40 + j) for j in range(T)]


def descriptors(T, n, seed=0, kept=False):
    """n descriptors over a bank of T: roots, power-0 parents at idx 0, children at every power, the table's two ends among the indices; with
    `kept` the kept form too -- to another index than its own, and one source named twice"""
    rs = np.random.RandomState(900 + 31 * T + 7 * n + seed)
    last = noise().size - P
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


def signed_zero_noise():
    """a table whose first 2 * 498 entries give a root every bias of which is -0.0 (scale_by is 0 there: the zero carries the noise's sign)"""
    n = noise().copy()
    n[:P] = -np.abs(n[:P])
    n[P:2 * P] = np.abs(n[P:2 * P])
    n.setflags(write=False)
    return n


# ---- the maze_ga_* surface without a GPU -------------------------------------------------------------------------------------------------------------
class MazeGaHostEngine(M.MazeHostEngine):
    """MazeHostEngine plus what ga_gpu.maze_main asks of a KIND_MAZE engine: the bank as a numpy array, thetas from the numpy statement above,
    episodes through dne_maze_rollout_host.  Every maze_ga_* call is recorded in self.calls; every evaluation's returns in self.evals."""

    def __init__(self, max_members=64, **kw):
        super().__init__(max_members=max_members, **kw)
        self.scale = None
        self.bank = np.zeros((0, P), np.float32)
        self.evals = []

    def _need(self, call, walls=False):
        from dne_hip import _lib
        if self.scale is None:
            raise _lib.DneError("%s: no init scale" % call)
        if self.noise is None:
            raise _lib.DneError("%s: noise table not uploaded" % call)
        if walls and self.maze is None:
            raise _lib.DneError("%s: no maze loaded" % call)

    def _check(self, call, parent, idx, kept):
        from dne_hip import _lib
        T = len(self.bank)
        if not 1 <= len(parent) <= self.max_members:
            raise _lib.DneError("%s: %d outside [1, max_members = %d]" % (call, len(parent), self.max_members))
        for a, b in zip(parent, idx):
            if a < -1 or a >= T or (a < 0 and b < 0) or (b < 0 and not kept) or b + P > self.noise.size:
                raise _lib.DneError("%s: descriptor (%d, %d) over %d parents and a table of %d" % (call, a, b, T, self.noise.size))

    def maze_ga_set_init_scale(self, sb):
        self.calls.append(("maze_ga_set_init_scale", ))
        self.scale = np.array(sb, np.float32)
        assert np.array_equal(M.bits(self.scale), M.bits(scale_by()))          # (the numpy statement above uses the model's own)

    def maze_ga_build(self, genomes):
        from dne_hip import _lib
        self._need("maze_ga_build")
        self.calls.append(("maze_ga_build", len(genomes)))
        if not 1 <= len(genomes) <= self.max_members or any(len(g) < 1 for g in genomes):
            raise _lib.DneError("maze_ga_build: %d genomes" % len(genomes))
        self.bank = np.stack([genome_theta(self.noise, g) for g in genomes])

    def maze_ga_eval(self, parent, idx, power, tslimit=M.STEPS):
        self._need("maze_ga_eval", walls=True)
        parent, idx = np.asarray(parent, np.int32).reshape(-1), np.asarray(idx, np.int64).reshape(-1)
        self.calls.append(("maze_ga_eval", len(parent)))
        self._check("maze_ga_eval", parent, idx, kept=False)
        out = self._run(list(members_theta(self.noise, self.bank, parent, idx, power)), tslimit)
        self.evals.append((parent.copy(), idx.copy(), out[0].copy(), out[2].copy()))
        return out

    def maze_ga_promote(self, parent, idx, power):
        self._need("maze_ga_promote")
        parent, idx = np.asarray(parent, np.int32).reshape(-1), np.asarray(idx, np.int64).reshape(-1)
        self.calls.append(("maze_ga_promote", len(parent)))
        self._check("maze_ga_promote", parent, idx, kept=True)
        self.bank = members_theta(self.noise, self.bank, parent, idx, power)

    def maze_ga_parents(self):
        return len(self.bank)

    def maze_ga_get_parent(self, j):
        return self.bank[j].copy()


# ---- the loop the reference's way ---------------------------------------------------------------------------------------------------------------------
class Individual(object):
    def __init__(self, seeds, reward, length):
        self.seeds, self.reward, self.length = seeds, reward, length


def plain_loop(noise_table, maze, exp, seed, iters, population=None):
    """gpu_implementation/ga.py:157-271 with nothing lazy: every offspring gets its genome, every theta -- offspring, validated individual,
    parent -- is rebuilt from its WHOLE genome each generation, the population is the full sorted list.  Shared with the driver by
    decision, not by code: the two whole-array draws per generation, and a previous elite's re-evaluation as theta + fl(0 * noise[0:498])
    while a bank exists.  -> one record per generation."""
    from dne_hip import _lib
    header, lines = maze
    n, T, V, k = exp["population_size"], exp["selection_threshold"], exp["validation_threshold"], exp["num_validation_episodes"]
    power, cutoff = exp["mutation_power"], exp["episode_cutoff_mode"]
    assert isinstance(cutoff, int) and not isinstance(power, dict)
    run = lambda thetas, limit: _lib.maze_rollout_host(np.stack(thetas), header, lines, min(limit, M.STEPS))[:2]
    rs = np.random.RandomState(seed)
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
        idx = rs.randint(0, noise_table.size - P + 1, size=n)
        tasks = [tuple(parents[of[i]]) + ((int(idx[i]), power), ) if parents else (int(idx[i]), ) for i in range(n)]
        rets, lens = run([genome_theta(noise_table, g) for g in tasks], cutoff)
        results = [Individual(g, float(r), int(l)) for g, r, l in zip(tasks, rets, lens)]
        population = sorted(results, key=lambda o: o.reward, reverse=True)          # stable: equal rewards keep arrival order
        validated = population[:V]
        thetas = [genome_theta(noise_table, o.seeds) for o in validated]
        if elite is not None:
            validated = [elite] + validated[:-1]
            again = genome_theta(noise_table, elite.seeds)
            thetas = [M.perturbed(again, noise_table, 0, 0.0) if parents else again] + thetas[:-1]
        vr, vl = zip(*(run([th] * k, cutoff) for th in thetas))
        val = [float(np.mean(r)) for r in vr]
        elite_at = int(np.argmax(val))
        elite = validated[elite_at]
        er, _ = run([thetas[elite_at]] * exp["num_test_episodes"], M.STEPS)
        timesteps += int(np.sum(lens)) + int(sum(np.sum(l) for l in vl))
        if np.mean(val) > best_val:
            best, best_val, best_test = elite.seeds, float(np.mean(val)), float(np.mean(er))
        parents = next_parents()
        records.append(dict(parents=list(parents), thetas=[genome_theta(noise_table, g) for g in parents], elite=elite.seeds,
                            returns=np.array(rets, np.float32), top=[o.seeds for o in population[:max(T, V)]], curr_solution=best,
                            curr_solution_val=best_val, curr_solution_test=best_test, timesteps_so_far=timesteps))
    return records
