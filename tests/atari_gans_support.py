"""TEST-ONLY support for GA-NS on Atari (csrc/ram_novelty.h): the pool-novelty contract over 128-byte RAM points restated
in plain Python (exact integer S, the distance through oracle.bc_distance on one-row arrays, sorted on (S, slot), a sequential sum), the
wrong-but-plausible forms the inputs must tell from it, the point sets both test files share, the dense numpy formulation with its derived
rounding bound, AtariGaNsHostEngine -- OracleEngine plus the new methods over the host twin and a Python archive, so that
ga_gpu.atari_ns_main runs without a GPU -- and plain_loop: GA-NS with nothing lazy, scored by the restatement."""
import functools
import math

import numpy as np

import oracle as O
from oracle_engine import OracleEngine

RAM, KMAX, TILE, MEMBERS = 128, 32, 256, 4           # bytes of a point; DNE_RAM_NOVELTY_KMAX, _TILE, _MEMBERS
S_MAX = RAM * 255 * 255                                # 8 323 200: all-0 against all-255
ARCHIVES = (0, 1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025)
COUNTS = (1, 2, 3, 5, 9, 33, 65)
KS = (1, 2, 25, 32)
# the device grid: the issue's archives, plus the kernel's tile size +-1 on both sides of the seam -- the archive ending one row before, on and
# one row after a tile boundary (255, 256, 257), and the population doing so (archive + n = 256 +- 1 for the n of the grid)
GPU_ARCHIVES = (0, 1, 31, 32, 33, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, TILE - 9, TILE - 10, TILE - 8, TILE - 33, TILE - 34, TILE - 32)
GPU_COUNTS = (1, 9, 33, 65)
GPU_KS = (1, 25, 32)
SETS = ("random", "lattice")


# ---- the contract, restated ------------------------------------------------------------------------------------------------------------------------
def squared(x, pool):
    """Python ints [len(pool)]: the exact sum of squared byte differences of x against every row of pool"""
    d = np.asarray(pool, np.uint8).astype(np.int64) - np.asarray(x, np.uint8).astype(np.int64)[None, :]
    return [int(v) for v in (d * d).sum(axis=1)]


def distance(x, y):
    """orc_bc_distance of two one-row trajectories"""
    return float(O.bc_distance(np.asarray(x, np.uint8).reshape(1, RAM), np.asarray(y, np.uint8).reshape(1, RAM)))


def ordered_pool(bc, archive, self_by="index", population_first=False):
    """Per member: every (combined slot, S) of its pool in the contract's order.  The pool is the archive at combined slots 0 .. A - 1, then the
    population at A .. A + n - 1, the member's own combined slot left out; sorted on (S, combined slot).  The keyword arguments make the
    WRONG forms (self_by "none" / "value", the population ahead of the archive in ties); the defaults are the contract."""
    bc = np.asarray(bc, np.uint8).reshape(-1, RAM)
    archive = np.zeros((0, RAM), np.uint8) if archive is None else np.asarray(archive, np.uint8).reshape(-1, RAM)
    pool = np.concatenate([archive, bc])
    A, n = len(archive), len(bc)
    out = []
    for m in range(n):
        S = squared(bc[m], pool)
        keyed = []
        for c in range(A + n):
            if self_by == "index" and c == A + m:
                continue
            if self_by == "value" and c >= A and S[c] == 0:
                continue
            tie = ((0, c - A) if c >= A else (1, c)) if population_first else (0, c)
            keyed.append((S[c], tie, c))
        out.append([(c, s) for s, _, c in sorted(keyed)])
    return out


def novelty_of(bc, archive, m, chosen, kk):
    """the distances of member m to the chosen combined slots added one by one, in order, into a double that starts at 0.0, divided by kk"""
    A = 0 if archive is None else len(archive)
    total = 0.0
    for c, _ in chosen:
        total += distance(bc[m], archive[c] if c < A else bc[c - A])
    return total / kk


def contract(bc, archive, k, kk_plus_self=False, ordered=None, **wrong):
    """(novelty float64 [n], neighbours int32 [n][kk]) of the contract, or of a wrong form"""
    bc = np.asarray(bc, np.uint8).reshape(-1, RAM)
    A, n = 0 if archive is None else len(archive), len(bc)
    kk = min(int(k), A + n if kk_plus_self else A + n - 1)
    ordered = ordered_pool(bc, archive, **wrong) if ordered is None else ordered
    nov = np.array([novelty_of(bc, archive, m, ordered[m][:kk], kk) for m in range(n)], np.float64)
    take = min(kk, min(len(o) for o in ordered))
    return nov, np.array([[c for c, _ in o[:take]] for o in ordered], np.int32).reshape(n, take)


WRONG_FORMS = {
    "self_not_excluded": dict(self_by="none"),
    "self_excluded_by_value": dict(self_by="value"),
    "kk_counts_self": dict(kk_plus_self=True),
    "population_before_archive_in_ties": dict(population_first=True),
}


# ---- the dense numpy formulation and its bound ----------------------------------------------------------------------------------------------------------
def dense_numpy(bc, archive, k):
    """concatenate, the n x (A + n) float64 matrix, mask the diagonal, np.partition, mean: what a host-side GA-NS generation would compute"""
    bc = np.asarray(bc, np.uint8).reshape(-1, RAM)
    archive = np.zeros((0, RAM), np.uint8) if archive is None else np.asarray(archive, np.uint8).reshape(-1, RAM)
    A, n = len(archive), len(bc)
    pool = np.concatenate([archive, bc]).astype(np.float64)
    x = bc.astype(np.float64)
    d = np.sqrt(((x[:, None, :] - pool[None, :, :]) ** 2).sum(axis=2))
    d[np.arange(n), A + np.arange(n)] = np.inf
    kk = min(int(k), A + n - 1)
    return np.partition(d, kk - 1, axis=1)[:, :kk].mean(axis=1)


def dense_bound(kk):
    """|contract - dense numpy| <= dense_bound(kk) * 2885, derived, not fitted.  Both sides select the same multiset of kk integers S (the order
    on S is exact on both: numpy's squared differences and their sums are exact integers below 2^53).  A distance is at most D = sqrt(S_MAX) <
    2885.  The contract's distance takes three roundings (sqrt, the product, the second sqrt): relative error <= u + u + u/2 + O(u^2) < 3u with
    u = 2^-53; numpy's takes one: <= u.  So each of the kk terms differs by at most 4u * D.  Each side adds kk terms with kk - 1 roundings of
    partial sums that are at most kk * D (numpy's pairwise order has no more roundings per term): <= 2 * (kk - 1) * u * kk * D in all.  The
    division rounds each side once: <= 2u * D after dividing.  Per unit of D:
        (kk * 4u + 2 * (kk - 1) * kk * u) / kk + 2u = (4 + 2 * (kk - 1) + 2) * u = (2 * kk + 4) * u,
    and a factor (1 + 2^-20) covers the O(u^2) terms."""
    u = 2.0 ** -53
    return (2 * kk + 4) * u * (1 + 2.0 ** -20)


D_MAX = 2885.0   # > sqrt(8 323 200) = 2884.99...


# ---- the point sets ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def point_set(name):
    """(members uint8 [65][128], archive uint8 [1025][128]); an archive of A points is its first A rows, a population of n its first n.
    random: seeded random bytes; member 1 sits on archive slot 0 and member 2 on member 0 (seen at n >= 3).
    lattice: bytes of {0, 1, 255} in the first three places, 0 elsewhere: 27 distinct points, so equal points and equal distances across the
    archive and the population are everywhere.  Member 0 is the origin, member 1 is e0 and archive slot 0 is e1: the origin's nearest are tied
    at S = 1 across the seam at every archive size >= 1."""
    rs = np.random.RandomState(1800 + SETS.index(name))
    if name == "random":
        mem = rs.randint(0, 256, (65, RAM)).astype(np.uint8)
        arch = rs.randint(0, 256, (1025, RAM)).astype(np.uint8)
        mem[1], mem[2] = arch[0], mem[0]
    else:
        vals = np.array([0, 1, 255], np.uint8)
        mem = np.zeros((65, RAM), np.uint8); arch = np.zeros((1025, RAM), np.uint8)
        mem[:, :3] = vals[rs.randint(0, 3, (65, 3))]
        arch[:, :3] = vals[rs.randint(0, 3, (1025, 3))]
        mem[0, :3] = (0, 0, 0); mem[1, :3] = (1, 0, 0); arch[0, :3] = (0, 1, 0)
    mem.setflags(write=False); arch.setflags(write=False)
    return mem, arch


def cell(name, A, n):
    mem, arch = point_set(name)
    return mem[:n], arch[:A]


def shapes(archives=ARCHIVES, counts=COUNTS):
    """every (A, n) of the grid but the refused pair"""
    return [(A, n) for A in archives for n in counts if A + n - 1 >= 1]


@functools.lru_cache(maxsize=None)
def ordered_cell(name, A, n):
    """ordered_pool of a cell, computed once (the k of a cell only cuts it)"""
    return ordered_pool(*cell(name, A, n))


@functools.lru_cache(maxsize=None)
def contract_cell(name, A, n, k):
    bc, arch = cell(name, A, n)
    return contract(bc, arch, k, ordered=ordered_cell(name, A, n))


@functools.lru_cache(maxsize=None)
def edge_cases():
    """name -> (bc, archive, tuple of k)"""
    rs = np.random.RandomState(1830)
    some = rs.randint(0, 256, (14, RAM)).astype(np.uint8)
    none = np.zeros((0, RAM), np.uint8)
    lo, hi = np.zeros((1, RAM), np.uint8), np.full((1, RAM), 255, np.uint8)
    on_point = some[:5].copy(); on_point[1] = some[8]                               # member 1 sits exactly on archive slot 3
    twins = some[:5].copy(); twins[3] = twins[0]
    return {
        "extremes": (np.concatenate([lo, hi, lo, some[:2]]), np.concatenate([hi, lo, some[5:7]]), (1, 2, 3, 8, 32)),   # S = 8 323 200
        "extremes_no_archive": (np.concatenate([lo, hi]), none, (1, 32)),
        "k_above_pool": (some[:3], some[5:7], (4, 5, 25, 32)),                       # A + n - 1 = 4
        "k_above_pool_no_archive": (some[:3], none, (2, 3, 32)),
        "member_on_an_archive_point": (on_point, some[5:], (1, 2, 11)),
        "two_members_equal": (twins, some[5:8], (1, 2, 7)),
        "two_members_equal_no_archive": (twins, none, (1, 2, 4)),
        "all_members_equal": (np.repeat(some[9:10], 5, axis=0), none, (1, 3, 4, 32)),
        "all_members_on_one_archive_point": (np.repeat(some[9:10], 5, axis=0), np.repeat(some[9:10], 2, axis=0), (1, 6, 32)),
    }


def all_inputs(archives=ARCHIVES, counts=COUNTS, ks=KS):
    """(name, bc, archive, k, (novelty, neighbours) of the contract) of everything the two test files score"""
    for name in SETS:
        for A, n in shapes(archives, counts):
            for k in ks:
                bc, arch = cell(name, A, n)
                yield (name, A, n), bc, arch, k, contract_cell(name, A, n, k)
    for name, (bc, archive, ks_) in sorted(edge_cases().items()):
        for k in ks_:
            yield name, bc, archive, k, contract(bc, archive, k)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the engine surface GA-NS asks for, without a GPU ------------------------------------------------------------------------------------------------
class AtariGaNsHostEngine(OracleEngine):
    """OracleEngine (kind KIND_GA by default) created as if with record_bc: ga_eval_powers keeps every member's final RAM, ram_novelty_pool
    scores through dne_ram_novelty_pool_host, the archive is a Python array.  Every pool score is kept in self.novelties."""

    def __init__(self, kind=1, record_bc=True, **kw):
        super().__init__(kind, **kw)
        self.record_bc = record_bc
        self._arch = np.zeros((0, RAM), np.uint8)
        self._last_bc = np.zeros((0, RAM), np.uint8)
        self.novelties = []

    def ga_eval_powers(self, genomes, tslimit, seeds, want_bc=False):
        self.calls.append(("ga_eval_powers", len(genomes)))
        out = [O.rollout(self.L, O.ga_gpu_rebuild(self.noise, g, self.scale_by), None, seeds[i], tslimit, want_bc=True) for i, g in enumerate(genomes)]
        r, s, l, bc = zip(*out)
        self._last_bc = np.stack(bc).astype(np.uint8)
        res = (np.array(r, np.float32), np.array(s, np.float32), np.array(l, np.int32))
        return res + (self._last_bc.copy(), ) if want_bc else res

    def ram_novelty_pool(self, k, bc=None, n=None, neighbours=False):
        from dne_hip import _lib
        self.calls.append(("ram_novelty_pool", int(k)))
        if not 1 <= int(k) <= KMAX:
            raise _lib.DneError("dne_ram_novelty_pool: k = %d outside 1..%d" % (k, KMAX))
        if bc is None:
            n = len(self._last_bc) if n is None else int(n)
            if not 1 <= n <= len(self._last_bc):
                raise _lib.DneError("dne_ram_novelty_pool: %d members asked for, the last evaluation ran %d" % (n, len(self._last_bc)))
            bc = self._last_bc[:n]
        out = _lib.ram_novelty_pool_host(bc, self._arch, k, neighbours=neighbours)
        self.novelties.append((out[0] if neighbours else out).copy())
        return out

    def archive_append_members(self, members):
        from dne_hip import _lib
        members = np.asarray(members, np.int32).reshape(-1)
        self.calls.append(("archive_append_members", len(members)))
        if len(members) < 1 or members.min() < 0 or members.max() >= len(self._last_bc):
            raise _lib.DneError("dne_archive_append_members: %r over the %d members of the last evaluation" % (members.tolist(), len(self._last_bc)))
        self._arch = np.concatenate([self._arch, self._last_bc[members]])

    def archive_get_points(self, first, count):
        from dne_hip import _lib
        if count < 1 or first < 0 or first + count > len(self._arch):
            raise _lib.DneError("dne_archive_get_points: entries %d .. %d asked for, the archive holds %d" % (first, first + count - 1, len(self._arch)))
        return self._arch[first:first + count].copy()

    def archive_size(self):
        return len(self._arch)

    def archive_clear(self):
        self._arch = np.zeros((0, RAM), np.uint8)

    def archive_append_points(self, points):
        self.calls.append(("archive_append_points", len(points)))
        self._arch = np.concatenate([self._arch, np.asarray(points, np.uint8).reshape(-1, RAM)])

    def ram_novelty_last_ms(self):
        return -1.0


# ---- GA-NS with nothing lazy --------------------------------------------------------------------------------------------------------------------------
def plain_loop(noise, exp, seed, iters, max_members=64, kind=1, nact=18):
    """GA-NS as ga_gpu.atari_ns_main's docstring decides it, written the long way: every theta is rebuilt from its whole genome, the final RAMs
    come back to the host, the novelty is the restatement above, the archive is a Python list.  The stream: parents (if any), indices, the
    archive mask, then the seeds of every evaluation call (at most max_members members each) in the order the calls are made.
    -> one record per generation."""
    from dne_hip import _lib, ga_gpu
    L = O.layout(kind, nact)
    sb = ga_gpu.model_scale_by(nact, kind)
    n, T, V, ve = exp["population_size"], exp["selection_threshold"], exp["validation_threshold"], exp["num_validation_episodes"]
    power, cutoff = exp["mutation_power"], exp["episode_cutoff_mode"]
    k, prob = exp["novelty_search"]["k"], exp["novelty_search"]["archive_prob"]
    assert isinstance(cutoff, int) and not isinstance(power, dict)
    rs = np.random.RandomState(seed)

    def run(genomes, limit):
        rets, lens, bcs = [], [], []
        for s in range(0, len(genomes), max_members):
            part = genomes[s:s + max_members]
            seeds = rs.randint(0, 2 ** 32, size=len(part), dtype=np.uint64).astype(np.uint32)
            for g, sd in zip(part, seeds):
                r, _, l, bc = O.rollout(L, O.ga_gpu_rebuild(noise, g, sb), None, sd, _lib.ENV_MAX_EPISODE_STEPS if limit is None else limit, want_bc=True)
                rets.append(r); lens.append(l); bcs.append(bc)
        return np.array(rets, np.float32), np.array(lens, np.int64), np.stack(bcs).astype(np.uint8)

    arch, parents, records = [], [], []
    best, best_val, best_test, timesteps = None, float("-inf"), float("-inf"), 0
    for g in range(iters):
        if parents:
            of = rs.randint(len(parents), size=n)
        idx = rs.randint(0, noise.size - L.P + 1, size=n)
        mask = rs.random_sample(n) < prob
        tasks = [tuple(parents[of[i]]) + ((int(idx[i]), power), ) if parents else (int(idx[i]), ) for i in range(n)]
        rets, lens, bc = run(tasks, cutoff)
        raw = contract(bc, np.array(arch, np.uint8).reshape(-1, RAM), k)[0]
        novelty = [v if math.isfinite(v) else 0.0 for v in raw]
        arch += [bc[i] for i in range(n) if mask[i]]
        by_novelty = sorted(range(n), key=lambda i: -novelty[i])                    # stable: equal novelties keep arrival order
        by_reward = sorted(range(n), key=lambda i: -float(rets[i]))
        validated = by_reward[:V]
        vr, vl, _ = run([tasks[i] for i in validated for _ in range(ve)], cutoff)
        val = [float(np.mean(vr[j * ve:(j + 1) * ve])) for j in range(len(validated))]
        elite = validated[int(np.argmax(val))]
        er = run([tasks[elite]] * exp["num_test_episodes"], None)[0]
        timesteps += int(np.sum(lens)) + int(np.sum(vl))
        if np.mean(val) > best_val:
            best, best_val, best_test = tasks[elite], float(np.mean(val)), float(np.mean(er))
        parents = [tasks[i] for i in by_novelty[:T]]
        records.append(dict(parents=list(parents), elite=tasks[elite], returns=rets, raw=np.array(raw, np.float64),
                            novelty=np.array(novelty, np.float64), archive=np.array(arch, np.uint8).reshape(-1, RAM), tasks=tasks, bc=bc,
                            curr_solution=best, curr_solution_val=best_val, curr_solution_test=best_test, timesteps_so_far=timesteps,
                            stream=rs.get_state()))
    return records


def exp(ns=None, **over):
    e = {"game": "frostbite", "model": "Model", "population_size": 6, "selection_threshold": 2, "validation_threshold": 2,
         "num_validation_episodes": 1, "num_test_episodes": 1, "episode_cutoff_mode": 12, "mutation_power": 0.005, "timesteps": 10 ** 9}
    e.update(over)
    e["novelty_search"] = dict({"k": 3, "archive_prob": 0.3}, **(ns or {}))
    return e


def same_stream(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def shared_noise(count=2_500_000):
    from dne_hip import es
    return es.SharedNoiseTable(count=count)
