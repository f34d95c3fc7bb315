"""TEST-ONLY support for GA-NS on the hard maze (csrc/maze_novelty.h's pool form): the pool-novelty contract as plain
Python, the wrong-but-plausible forms the inputs must tell from it, a dense numpy formulation for the derived bound, the inputs every test
file shares, MazeGaNsHostEngine -- MazeGaHostEngine plus the archive and the pool novelty through dne_maze_novelty_pool_host, so that
dne_hip/ga_gpu.py's GA-NS loop runs without a GPU -- and plain_loop: GA-NS with nothing lazy, scored by the Python contract."""
import functools
import math

import numpy as np

import maze_ga_support as G
import maze_novelty_support as N
import maze_support as M

P = M.P
KMAX, TILE = N.KMAX, N.TILE
ARCHIVES = (0, 1, 2, 63, 64, 65, TILE - 4, TILE - 1, TILE, TILE + 1)   # 1020 + 9 members: the population across the tile boundary
COUNTS = (1, 2, 3, 4, 5, 9)                                              # four members per workgroup, a partial last one
KS = (1, 2, 25, 32)
NAN, INF = N.NAN, N.INF


# ---- the contract, in plain Python ------------------------------------------------------------------------------------------------------------
def _distance(px, py, qx, qy):
    dx, dy = qx - px, qy - py
    s = dx * dx + dy * dy
    return math.sqrt(s) if s == s else NAN               # (math.sqrt(inf) is inf; a NaN stays a NaN)


def neighbours(xy, archive, k, self_by="index", population_first=False, kk_plus_self=False):
    """Per member: the (combined slot, distance) pairs its novelty is made of, in order.  The pool is the archive at combined slots 0 .. A - 1,
    then the population at A .. A + n - 1, the member's own combined slot left out; sorted on (isnan, value, combined slot); the first
    kk = min(k, A + n - 1).  The keyword arguments make the WRONG forms (self_by "none" / "value" / "value_everywhere", the population ahead of the archive in
    ties, kk = min(k, A + n)); the defaults are the contract."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    archive = np.zeros((0, 2), np.float32) if archive is None else np.asarray(archive, np.float32).reshape(-1, 2)
    pts = [(float(a[0]), float(a[1])) for a in archive] + [(float(p[0]), float(p[1])) for p in xy]
    A, n = len(archive), len(xy)
    out = []
    for p in range(n):
        px, py = pts[A + p]
        keyed = []
        for c, (qx, qy) in enumerate(pts):
            if self_by == "index" and c == A + p:
                continue
            if self_by == "value" and c >= A and (qx, qy) == (px, py):
                continue
            if self_by == "value_everywhere" and (qx, qy) == (px, py):
                continue
            d = _distance(px, py, qx, qy)
            tie = ((0, c - A) if c >= A else (1, c)) if population_first else (0, c)
            keyed.append((d != d, 0.0 if d != d else d, tie, c, d))
        kk = min(int(k), A + n if kk_plus_self else A + n - 1)
        out.append(([(c, d) for _, _, _, c, d in sorted(keyed)[:kk]], kk))
    return out


def contract(xy, archive, k, **wrong):
    """the novelty: the neighbours' distances added one by one, in order, into a double that starts at 0.0, divided by kk"""
    out = []
    for chosen, kk in neighbours(xy, archive, k, **wrong):
        total = 0.0
        for _, d in chosen:
            total += d
        out.append(total / kk if kk else NAN)
    return np.array(out, np.float64)


WRONG_FORMS = {
    "self_not_excluded": dict(self_by="none"),
    "self_excluded_by_value": dict(self_by="value"),
    "everything_at_distance_zero_excluded": dict(self_by="value_everywhere"),
    "population_before_archive_in_ties": dict(population_first=True),
    "kk_counts_self": dict(kk_plus_self=True),
}


# ---- a dense numpy formulation: archive and population concatenated, the diagonal masked -----------------------------------------------------------
def dense_np(xy, archive, k):
    """what a host-side GA-NS would write: one [n][A + n] float64 matrix, the member's own column set to +inf, a sort per row, a mean"""
    xy = np.asarray(xy, np.float32).astype(np.float64).reshape(-1, 2)
    archive = np.asarray(archive, np.float32).astype(np.float64).reshape(-1, 2)
    pool = np.concatenate([archive, xy])
    d = np.sqrt(((xy[:, None, :] - pool[None, :, :]) ** 2).sum(-1))
    d[np.arange(len(xy)), len(archive) + np.arange(len(xy))] = np.inf
    kk = min(k, len(pool) - 1)
    return np.sort(d, axis=1)[:, :kk].mean(axis=1)


@functools.lru_cache(maxsize=None)
def dense_cases():
    """archives of 0 .. 120 points with 9 members in [0, 300)^2: (xy, archive) pairs, none set aside"""
    rs = np.random.RandomState(2025)
    cases = []
    for narch in range(0, 121):
        archive = rs.uniform(0, 300, (narch, 2)).astype(np.float32)
        xy = rs.uniform(0, 300, (9, 2)).astype(np.float32)
        if narch:
            xy[0] = archive[rs.randint(narch)]
        xy[5] = xy[3]
        cases.append((xy, archive))
    return cases


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------------------
def archive(A):
    return N.sized_archive(A) if A else np.zeros((0, 2), np.float32)


@functools.lru_cache(maxsize=None)
def members():
    """9 members: 0 sits on archive slot 0 of every sized archive, 6 sits on member 2 (two members at one point), 7 on archive slot 1"""
    xy = N.members().copy()
    xy[6] = xy[2]
    xy[7] = N.sized_archive(2)[1]
    xy.setflags(write=False)
    return xy


def shapes():
    """every (A, n) of the issue but the refused pair"""
    return [(A, n) for A in ARCHIVES for n in COUNTS if A + n - 1 >= 1]


@functools.lru_cache(maxsize=None)
def edge_cases():
    """name -> (xy, archive, tuple of k)"""
    rs = np.random.RandomState(17)
    f = lambda *rows: np.array(rows, np.float32).reshape(-1, 2)
    some = rs.uniform(0, 300, (12, 2)).astype(np.float32)
    none = np.zeros((0, 2), np.float32)
    on_point = some[:5].copy(); on_point[1] = some[8]                               # member 1 sits exactly on archive slot 8
    twins = some[:5].copy(); twins[3] = twins[0]
    nan_member = some[:6].copy(); nan_member[2] = (NAN, 1.0)
    nan_arch = some.copy(); nan_arch[[1, 4]] = f((NAN, 5.0), (NAN, NAN))
    lat = N.lattice()
    origin = int(np.flatnonzero((lat == 0).all(1))[0])
    ring = [int(i) for i in np.flatnonzero(np.abs(lat).sum(1) == 1)]               # the four points at distance 1
    diag = [int(i) for i in np.flatnonzero((np.abs(lat) == 1).all(1))]             # the four at sqrt 2
    lattice_xy = lat[[origin, ring[1], ring[2], diag[0], diag[3]]]                 # the origin and some of its tied neighbours are MEMBERS,
    lattice_arch = np.delete(lat, [origin, ring[1], ring[2], diag[0], diag[3]], axis=0)   # the others of each ring are in the archive
    return {
        "k_above_pool": (some[:3], some[5:7], (4, 5, 25, 32)),                       # A + n - 1 = 4
        "k_above_pool_no_archive": (some[:3], none, (2, 3, 32)),
        "member_on_an_archive_point": (on_point, some[5:], (1, 2, 11)),
        "two_members_at_one_point": (twins, some[5:8], (1, 2, 7)),
        "two_members_at_one_point_no_archive": (twins, none, (1, 2, 4)),
        "all_members_at_one_point": (np.repeat(f((10, 10)), 5, axis=0), none, (1, 3, 4, 32)),
        "all_members_on_one_archive_point": (np.repeat(f((10, 10)), 5, axis=0), f((10, 10), (10, 10)), (1, 6, 32)),
        "lattice": (lattice_xy, lattice_arch, (1, 2, 3, 4, 5, 7, 8, 9, 12, 32)),
        "tiny_and_huge": (f((0, 0), (1e-30, -1e-30), (1e30, 1e30), (1, 1)), f((1e-30, 0), (0, 1e-30), (1e30, -1e30), (3e38, 3e38), (1e-38, 1e-45)), (1, 2, 3, 8)),
        "inf": (f((INF, 0), (-INF, INF), (1, 1), (2, 2)), np.concatenate([some[:3], f((INF, 0), (-INF, 3))]), (1, 3, 4, 5, 8)),   # inf - inf: a NaN distance
        "nan_member": (nan_member, some[6:10], (1, 8, 9, 32)),                       # nine in a pool, eight numbers for the others: kk = 9 reaches the NaN
        "nan_member_no_archive": (nan_member, none, (1, 4, 5)),
        "nan_archive_entries": (some[:4], nan_arch, (1, 12, 13, 14, 15)),            # 13 numbers (10 archive + 3 members), then the two NaNs
    }


def same(a, b):
    return N.same(a, b)


# ---- the engine surface GA-NS asks for, without a GPU ----------------------------------------------------------------------------------------------
class MazeGaNsHostEngine(G.MazeGaHostEngine, N.MazeNoveltyHostEngine):
    """MazeGaHostEngine (the bank, maze_ga_*) and MazeNoveltyHostEngine (the archive) plus maze_novelty_pool through dne_maze_novelty_pool_host
    and maze_archive_append_members.  Every pool score is kept in self.novelties."""

    def __init__(self, max_members=64, **kw):
        super().__init__(max_members=max_members, **kw)
        self.novelties = []

    def maze_novelty_pool(self, k, xy=None, n=None):
        from dne_hip import _lib
        self.calls.append(("maze_novelty_pool", int(k)))
        if not 1 <= int(k) <= KMAX:
            raise _lib.DneError("maze_novelty_pool: k = %d outside 1..%d" % (k, KMAX))
        out = _lib.maze_novelty_pool_host(self._points("maze_novelty_pool", xy, n), self._arch, k)
        self.novelties.append(out.copy())
        return out

    def maze_final_state(self, n):
        self.calls.append(("maze_final_state", int(n)))
        return super().maze_final_state(n)

    def maze_novelty(self, k, xy=None, n=None):
        self.calls.append(("maze_novelty", int(k)))
        return super().maze_novelty(k, xy=xy, n=n)

    def maze_archive_append_members(self, members):
        from dne_hip import _lib
        members = np.asarray(members, np.int32).reshape(-1)
        self.calls.append(("maze_archive_append_members", len(members)))
        if len(members) < 1 or members.min() < 0 or members.max() >= self._last_n:
            raise _lib.DneError("maze_archive_append_members: %r over the %d members of the last evaluation" % (members.tolist(), self._last_n))
        self._arch = np.concatenate([self._arch, self._xy[members]])


# ---- GA-NS with nothing lazy ---------------------------------------------------------------------------------------------------------------------
def plain_loop(noise_table, maze, exp, seed, iters, poison=None):
    """GA-NS as dne_hip/ga_gpu.py's docstring decides it, written the long way: every offspring gets its genome, every theta -- offspring,
    validated individual, parent -- is rebuilt from its WHOLE genome each generation, the final positions come back to the host, the novelty
    is the Python contract above, the archive is a Python list.  `poison` (generation, member) -> a theta to run in that member's place (how a
    NaN policy is put into a run).  -> one record per generation."""
    from dne_hip import _lib
    header, lines = maze
    n, T, V, ve = exp["population_size"], exp["selection_threshold"], exp["validation_threshold"], exp["num_validation_episodes"]
    power, cutoff = exp["mutation_power"], exp["episode_cutoff_mode"]
    k, prob = exp["novelty_search"]["k"], exp["novelty_search"]["archive_prob"]
    assert isinstance(cutoff, int) and not isinstance(power, dict)
    run = lambda thetas, limit: _lib.maze_rollout_host(np.stack(thetas), header, lines, min(limit, M.STEPS))
    rs = np.random.RandomState(seed)
    arch, parents, records = [], [], []
    best, best_val, best_test, timesteps = None, float("-inf"), float("-inf"), 0
    for g in range(iters):
        if parents:
            of = rs.randint(len(parents), size=n)
        idx = rs.randint(0, noise_table.size - P + 1, size=n)
        mask = rs.random_sample(n) < prob
        tasks = [tuple(parents[of[i]]) + ((int(idx[i]), power), ) if parents else (int(idx[i]), ) for i in range(n)]
        thetas = [G.genome_theta(noise_table, t) for t in tasks]
        if poison and poison[0] == g:
            thetas[poison[1]] = poison[2]
        rets, lens, xy = run(thetas, cutoff)
        raw = contract(xy, np.array(arch, np.float32).reshape(-1, 2), k)
        novelty = [v if math.isfinite(v) else 0.0 for v in raw]
        arch += [tuple(xy[i]) for i in range(n) if mask[i]]
        by_novelty = sorted(range(n), key=lambda i: -novelty[i])                    # stable: equal novelties keep arrival order
        by_reward = sorted(range(n), key=lambda i: -float(rets[i]))
        validated = by_reward[:V]
        vr, vl, _ = zip(*(run([thetas[i]] * ve, cutoff) for i in validated))
        val = [float(np.mean(r)) for r in vr]
        elite = validated[int(np.argmax(val))]
        er = run([thetas[elite]] * exp["num_test_episodes"], M.STEPS)[0]
        timesteps += int(np.sum(lens)) + int(sum(np.sum(l) for l in vl))
        if np.mean(val) > best_val:
            best, best_val, best_test = tasks[elite], float(np.mean(val)), float(np.mean(er))
        parents = [tasks[i] for i in by_novelty[:T]]
        records.append(dict(parents=list(parents), thetas=[thetas[i] for i in by_novelty[:T]], elite=tasks[elite],
                            returns=np.array(rets, np.float32), raw=np.array(raw, np.float64), novelty=np.array(novelty, np.float64),
                            archive=np.array(arch, np.float32).reshape(-1, 2), tasks=tasks, by_novelty=by_novelty, by_reward=by_reward, xy=np.array(xy),
                            validated=[tasks[i] for i in validated], curr_solution=best, curr_solution_val=best_val,
                            curr_solution_test=best_test, timesteps_so_far=timesteps))
    return records
