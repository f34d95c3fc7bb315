"""TEST-ONLY support for GA-NS on the dense kind (csrc/dense_novelty.h's pool form): the pool-novelty contract with D
floats a point restated in plain Python / numpy, the wrong-but-plausible forms the inputs must tell from it, the point sets both test files
share, DenseGaNsHostEngine -- DenseGaHostEngine (the bank) plus DenseNoveltyHostEngine (BCs, archive, dense_novelty) plus the pool twin and
the gather, so that ga_gpu.dense_ns_main runs without a GPU -- and plain_loop: GA-NS with nothing lazy, every genome kept, every theta rebuilt
from its whole genome, scored by the restatement.  Every comparison is bit for bit."""
import functools
import math

import numpy as np

import dense_ga_support as G
import dense_novelty_support as N
import dense_support as D
import maze_support as M
import stepenv_support as SS

KMAX, TILE = N.KMAX, N.TILE
DIMS = (2, 4)
ARCHIVES = (0, 1, 2, 63, 64, 65, TILE - 4, TILE - 1, TILE, TILE + 1)   # 1020 + 9 members: the population across the tile boundary
GPU_ARCHIVES = (0, 1, 63, 64, 65, TILE - 4, TILE, TILE + 1)
COUNTS = (1, 2, 3, 4, 5, 9)                                              # four members per workgroup, a partial last one
KS = (1, 2, 25, 32)
SETS = ("lattice", "random")
NAN, INF = np.float32("nan"), np.float32("inf")
same, bits = N.same, N.bits


# ---- the contract, restated ------------------------------------------------------------------------------------------------------------------------
def distances(p, pool):
    """float64 [len(pool)]: d_i = q_i - p_i in double, s = d_0 * d_0, then s = s + d_i * d_i for i ascending, np.sqrt (correctly rounded)"""
    Q, p = np.asarray(pool, np.float32).astype(np.float64), np.asarray(p, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d = Q[:, 0] - p[0]
        s = d * d
        for i in range(1, Q.shape[1]):
            d = Q[:, i] - p[i]
            s = s + d * d
        return np.sqrt(s)


def ordered_pool(bc, archive, self_by="index", population_first=False):
    """Per member: every (combined slot, distance) of its pool in the contract's order.  The pool is the archive at combined slots 0 .. A - 1,
    then the population at A .. A + n - 1, the member's own combined slot left out; sorted on (isnan, value, combined slot).  The keyword
    arguments make the WRONG forms (self_by "none" / "value", the population ahead of the archive in ties); the defaults are the contract."""
    bc = np.asarray(bc, np.float32)
    dim = bc.shape[1]
    archive = np.zeros((0, dim), np.float32) if archive is None else np.asarray(archive, np.float32).reshape(-1, dim)
    pool = np.concatenate([archive, bc])
    A, n = len(archive), len(bc)
    out = []
    for p in range(n):
        dist = distances(bc[p], pool)
        keyed = []
        for c in range(A + n):
            if self_by == "index" and c == A + p:
                continue
            if self_by == "value" and c >= A and bits(pool[c]).tolist() == bits(bc[p]).tolist():
                continue
            d = float(dist[c])
            tie = ((0, c - A) if c >= A else (1, c)) if population_first else (0, c)
            keyed.append((d != d, 0.0 if d != d else d, tie, c, d))
        out.append([(c, d) for _, _, _, c, d in sorted(keyed)])
    return out


def neighbours(bc, archive, k, kk_plus_self=False, **wrong):
    """per member (the kk first (combined slot, distance) pairs of its pool's order, kk); kk = min(k, A + n - 1)"""
    A, n = 0 if archive is None else len(archive), len(bc)
    kk = min(int(k), A + n if kk_plus_self else A + n - 1)
    return [(chosen[:kk], kk) for chosen in ordered_pool(bc, archive, **wrong)]


def novelty_of(chosen, kk):
    """the distances added one by one, in order, into a double that starts at 0.0, divided by kk"""
    total = 0.0
    for _, d in chosen:
        total += d
    with np.errstate(all="ignore"):
        return float(np.float64(total) / np.float64(kk)) if kk else float("nan")


def contract(bc, archive, k, **wrong):
    return np.array([novelty_of(chosen, kk) for chosen, kk in neighbours(bc, archive, k, **wrong)], np.float64)


WRONG_FORMS = {
    "self_not_excluded": dict(self_by="none"),
    "self_excluded_by_value": dict(self_by="value"),
    "kk_counts_self": dict(kk_plus_self=True),
    "population_before_archive_in_ties": dict(population_first=True),
}


# ---- the point sets ---------------------------------------------------------------------------------------------------------------------------------
def _unit(dim, axis, sign=1.0):
    v = np.zeros(dim, np.float32)
    v[axis] = sign
    return v


@functools.lru_cache(maxsize=None)
def point_set(name, dim):
    """(members float32 [9][dim], archive float32 [TILE + 1][dim]); an archive of A points is its first A rows.
    lattice: integer coordinates in -3 .. 3.  Member 0 is the origin, members 1, 2, 3 are +e0, -e0, +e1 and archive slot 0 is -e1; no archive
    point is the origin (such draws become -e1 too).  So the origin's nearest are tied at distance 1 across the archive and the population, at
    every archive size >= 1.  Member 6 sits on member 4 (two members at one BC), member 7 on archive slot 1.
    random: uniform in [-10, 10); member 0 sits on archive slot 0, member 6 on member 2, member 7 on archive slot 1."""
    rs = np.random.RandomState(700 + 10 * dim + SETS.index(name))
    if name == "lattice":
        mem = rs.randint(-3, 4, (9, dim)).astype(np.float32)
        arch = rs.randint(-3, 4, (TILE + 1, dim)).astype(np.float32)
        mem[0] = 0
        mem[1], mem[2], mem[3] = _unit(dim, 0), _unit(dim, 0, -1.0), _unit(dim, 1)
        arch[(arch == 0).all(1)] = _unit(dim, 1, -1.0)
        arch[0] = _unit(dim, 1, -1.0)
        mem[6] = mem[4]
        mem[7] = arch[1]
    else:
        mem = rs.uniform(-10, 10, (9, dim)).astype(np.float32)
        arch = rs.uniform(-10, 10, (TILE + 1, dim)).astype(np.float32)
        mem[0], mem[6], mem[7] = arch[0], mem[2], arch[1]
    mem.setflags(write=False); arch.setflags(write=False)
    return mem, arch


def cell(name, dim, A, n):
    mem, arch = point_set(name, dim)
    return mem[:n], arch[:A]


def shapes(archives=ARCHIVES):
    """every (A, n) of the grid but the refused pair"""
    return [(A, n) for A in archives for n in COUNTS if A + n - 1 >= 1]


@functools.lru_cache(maxsize=None)
def ordered_cell(name, dim, A, n):
    """ordered_pool of a cell, computed once (the k of a cell only cuts it)"""
    return ordered_pool(*cell(name, dim, A, n))


def contract_cell(name, dim, A, n, k):
    kk = min(k, A + n - 1)
    return np.array([novelty_of(chosen[:kk], kk) for chosen in ordered_cell(name, dim, A, n)], np.float64)


def tie_across_the_cut(name, dim, A, n, ks=KS):
    """does some member of the cell have equal distances on both sides of position kk, for some k of the grid, with points of the archive AND
    of the population among those at that distance"""
    for chosen in ordered_cell(name, dim, A, n):
        for k in ks:
            if k < len(chosen) and chosen[k - 1][1] == chosen[k][1]:
                tied = [c for c, d in chosen if d == chosen[k][1]]
                if any(c < A for c in tied) and any(c >= A for c in tied):
                    return True
    return False


@functools.lru_cache(maxsize=None)
def edge_cases(dim):
    """name -> (bc, archive, tuple of k), every point of `dim` floats"""
    rs = np.random.RandomState(17 + dim)
    f = lambda *rows: np.array([np.broadcast_to(np.asarray(r, np.float32), (dim, )) for r in rows], np.float32).reshape(-1, dim)
    some = rs.uniform(-10, 10, (12, dim)).astype(np.float32)
    none = np.zeros((0, dim), np.float32)
    last = lambda v, w: np.concatenate([np.full(dim - 1, v, np.float32), np.array([w], np.float32)])
    on_point = some[:5].copy(); on_point[1] = some[8]                               # member 1 sits exactly on archive slot 8
    twins = some[:5].copy(); twins[3] = twins[0]
    nan_member = some[:6].copy(); nan_member[2, dim - 1] = NAN
    nan_arch = some.copy(); nan_arch[1, 0] = NAN; nan_arch[4] = NAN
    zeros = f(0.0, -0.0, last(0.0, -0.0), last(-0.0, 0.0))                           # four members at one point, written four ways
    return {
        "k_above_pool": (some[:3], some[5:7], (4, 5, 25, 32)),                       # A + n - 1 = 4
        "k_above_pool_no_archive": (some[:3], none, (2, 3, 32)),
        "member_on_an_archive_point": (on_point, some[5:], (1, 2, 11)),
        "two_members_at_one_bc": (twins, some[5:8], (1, 2, 7)),
        "two_members_at_one_bc_no_archive": (twins, none, (1, 2, 4)),
        "all_members_at_one_bc": (np.repeat(f(10.0), 5, axis=0), none, (1, 3, 4, 32)),
        "all_members_on_one_archive_point": (np.repeat(f(10.0), 5, axis=0), f(10.0, 10.0), (1, 6, 32)),
        "signed_zeros": (zeros, f(-0.0, last(0.0, 1.0)), (1, 3, 4, 5)),
        "tiny_and_huge": (f(0.0, 1e-40, 1e30, 1.0, last(1e30, -1e30)), f(last(1e-40, 0.0), 1e30, -1e30, 3e38, last(1e-38, 1e-45)), (1, 2, 3, 8, 9)),
        "inf": (f(last(0.0, INF), last(INF, -INF), 1.0, 2.0), np.concatenate([some[:3], f(last(0.0, INF), last(3.0, -INF))]), (1, 3, 4, 5, 8)),
        "nan_member": (nan_member, some[6:10], (1, 8, 9, 32)),                       # nine in a pool, eight numbers for the others: kk = 9 reaches the NaN
        "nan_member_no_archive": (nan_member, none, (1, 4, 5)),
        "nan_archive_points": (some[:4], nan_arch, (1, 12, 13, 14, 15)),             # 13 numbers (10 archive + 3 members), then the two NaNs
    }


def all_inputs(dim, archives=ARCHIVES):
    """(name, bc, archive, k) of everything the two test files score at `dim`"""
    for name in SETS:
        for A, n in shapes(archives):
            for k in KS:
                yield (name, A, n), cell(name, dim, A, n)[0], cell(name, dim, A, n)[1], k
    for name, (bc, archive, ks) in sorted(edge_cases(dim).items()):
        for k in ks:
            for n in sorted(set(min(n, len(bc)) for n in COUNTS)):
                if len(archive) + n - 1 >= 1:
                    yield name, bc[:n], archive, k


# ---- the engine surface GA-NS asks for, without a GPU ------------------------------------------------------------------------------------------------
class DenseGaNsHostEngine(G.DenseGaHostEngine, N.DenseNoveltyHostEngine):
    """DenseGaHostEngine (the bank, dense_ga_*) and DenseNoveltyHostEngine (BCs, archive, dense_novelty) plus dense_novelty_pool through
    dne_dense_novelty_pool_host and dense_archive_append_members.  Every pool score is kept in self.novelties."""

    def __init__(self, env, hidden=(), nonlin="relu", max_members=16, **kw):
        super().__init__(env, hidden, nonlin, max_members, **kw)
        self.novelties = []

    def dense_novelty_pool(self, k, bc=None, n=None):
        from dne_hip import _lib
        self.calls.append(("dense_novelty_pool", int(k)))
        if not 1 <= int(k) <= KMAX:
            raise _lib.DneError("dne_dense_novelty_pool: k = %d outside 1..%d" % (k, KMAX))
        out = _lib.dense_novelty_pool_host(self._points("dne_dense_novelty_pool", bc, n), self._arch, k, D=self.dim)
        self.novelties.append(out.copy())
        return out

    def dense_final_state(self, n):
        self.calls.append(("dense_final_state", int(n)))
        return super().dense_final_state(n)

    def dense_novelty(self, k, bc=None, n=None):
        self.calls.append(("dense_novelty", int(k)))
        return super().dense_novelty(k, bc=bc, n=n)

    def dense_archive_append_members(self, members):
        from dne_hip import _lib
        members = np.asarray(members, np.int32).reshape(-1)
        self.calls.append(("dense_archive_append_members", len(members)))
        if len(members) < 1 or members.min() < 0 or members.max() >= self._last_n:
            raise _lib.DneError("dne_dense_archive_append_members: %r over the %d members of the last evaluation" % (members.tolist(), self._last_n))
        self._arch = np.concatenate([self._arch, _lib.dense_bc_host(self.env_kind, self._state[:self._last_n])[members]])


def host_engine(case, max_members=10, cls=DenseGaNsHostEngine):
    env, hidden, nl = case
    e = cls(env, hidden, nl, max_members)
    if env == "maze":
        e.maze_set_walls(*M.fixture_maze())
    e.noise_upload(G.noise())
    return e


# ---- GA-NS with nothing lazy --------------------------------------------------------------------------------------------------------------------------
def plain_loop(case, exp, seed, iters, poison=None, max_members=10):
    """GA-NS as ga_gpu.dense_ns_main's docstring decides it, written the long way: every offspring gets its genome, every theta -- offspring,
    validated individual, parent -- is rebuilt from its WHOLE genome each generation, the final state records come back to the host, the BC is
    their first D doubles cast to float32, the novelty is the restatement above, the archive is a Python list.  The stream: parents (if any),
    indices, the archive mask; on the cart-pole the seeds of every evaluation call (at most max_members members each) follow, in the order the
    calls are made.  `poison` (generation, member, theta): a theta to run in that member's place.  -> one record per generation."""
    env = case[0]
    table, sb, P, dim = G.noise(), G.scale_by(case), G.num_params(case), N.BC_DIM[env]
    n, T, V, ve = exp["population_size"], exp["selection_threshold"], exp["validation_threshold"], exp["num_validation_episodes"]
    power, cutoff = exp["mutation_power"], exp["episode_cutoff_mode"]
    k, prob = exp["novelty_search"]["k"], exp["novelty_search"]["archive_prob"]
    assert isinstance(cutoff, int) and not isinstance(power, dict)
    rs = np.random.RandomState(seed)

    def run(thetas, limit):
        rets, lens, states = [], [], []
        for s in range(0, len(thetas), max_members):
            part = thetas[s:s + max_members]
            seeds = None if env == "maze" else rs.randint(0, 2 ** 32, size=len(part), dtype=np.uint64).astype(np.uint32)
            r = G.rollout(case, np.stack(part), limit, seeds)
            rets.append(r["returns"]); lens.append(r["lengths"]); states.append(r["state"])
        return np.concatenate(rets), np.concatenate(lens), np.concatenate(states)

    arch, parents, records = [], [], []
    best, best_val, best_test, timesteps = None, float("-inf"), float("-inf"), 0
    for g in range(iters):
        if parents:
            of = rs.randint(len(parents), size=n)
        idx = rs.randint(0, table.size - P + 1, size=n)
        mask = rs.random_sample(n) < prob
        tasks = [tuple(parents[of[i]]) + ((int(idx[i]), power), ) if parents else (int(idx[i]), ) for i in range(n)]
        thetas = [G.genome_theta(table, sb, t) for t in tasks]
        if poison and poison[0] == g:
            thetas[poison[1]] = poison[2]
        rets, lens, state = run(thetas, cutoff)
        bc = state[:, :dim].astype(np.float32)
        raw = contract(bc, np.array(arch, np.float32).reshape(-1, dim), k)
        novelty = [v if math.isfinite(v) else 0.0 for v in raw]
        arch += [bc[i] for i in range(n) if mask[i]]
        by_novelty = sorted(range(n), key=lambda i: -novelty[i])                    # stable: equal novelties keep arrival order
        by_reward = sorted(range(n), key=lambda i: -float(rets[i]))
        validated = by_reward[:V]
        vr, vl, _ = run([thetas[i] for i in validated for _ in range(ve)], cutoff)
        val = [float(np.mean(vr[j * ve:(j + 1) * ve])) for j in range(len(validated))]
        elite = validated[int(np.argmax(val))]
        er = run([thetas[elite]] * exp["num_test_episodes"], 0)[0]
        timesteps += int(np.sum(lens)) + int(np.sum(vl))
        if np.mean(val) > best_val:
            best, best_val, best_test = tasks[elite], float(np.mean(val)), float(np.mean(er))
        parents = [tasks[i] for i in by_novelty[:T]]
        records.append(dict(parents=list(parents), thetas=[thetas[i] for i in by_novelty[:T]], elite=tasks[elite],
                            returns=np.array(rets, np.float32), raw=np.array(raw, np.float64), novelty=np.array(novelty, np.float64),
                            archive=np.array(arch, np.float32).reshape(-1, dim), tasks=tasks, by_novelty=by_novelty, by_reward=by_reward, bc=bc,
                            validated=[tasks[i] for i in validated], curr_solution=best, curr_solution_val=best_val,
                            curr_solution_test=best_test, timesteps_so_far=timesteps, stream=rs.get_state()))
    return records


def exp(game, model="LinearClassifier", ns=None, **over):
    e = G.exp(game, model, **over)
    e["novelty_search"] = dict({"k": 3, "archive_prob": 0.3}, **(ns or {}))
    return e


def same_stream(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


shared_noise = D.shared_noise
log_rows = D.log_rows
kind_id = SS.kind_id
