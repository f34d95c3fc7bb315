"""TEST-ONLY support for novelty on the hard maze (csrc/maze_novelty.h): the contract as plain Python, the reference's
formula in numpy, the tolerance between the two (derived below, not fitted), the inputs every test file shares, and MazeNoveltyHostEngine --
MazeHostEngine plus the archive and maze_novelty through dne_maze_novelty_host, so that dne_hip/nses_gpu.py runs without a GPU."""
import functools
import math

import numpy as np

import maze_support as M

KMAX, TILE = 32, 1024                      # DNE_MAZE_NOVELTY_KMAX; archive points per LDS tile of k_maze_novelty (tests check them against _lib)
SIZES = (1, 2, 9, 10, 11, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
KS = (1, 2, 10, 31, 32)
COUNTS = (1, 3, 4, 5, 9)                   # members: below, at and above the kernel's four per workgroup
NAN, INF = float("nan"), float("inf")


# ---- the contract, in plain Python -----------------------------------------------------------------------------------------------------------
def contract(xy, archive, k):
    """Python floats (doubles), math.sqrt (correctly rounded), sorted on (isnan, value, slot), a sequential sum from 0.0, one division"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2); archive = np.asarray(archive, np.float32).reshape(-1, 2)
    arch = [(float(a[0]), float(a[1])) for a in archive]
    kk = min(int(k), len(arch))
    out = []
    for p in xy:
        px, py = float(p[0]), float(p[1])
        keyed = []
        for slot, (ax, ay) in enumerate(arch):
            dx, dy = ax - px, ay - py
            s = dx * dx + dy * dy
            d = math.sqrt(s) if s == s else NAN          # (math.sqrt(inf) is inf; a NaN stays a NaN)
            keyed.append((d != d, 0.0 if d != d else d, slot, d))
        total = 0.0
        for _, _, _, d in sorted(keyed)[:kk]:
            total += d
        out.append(total / kk)
    return np.array(out, np.float64)


# ---- nses.py:12-32 in numpy, written from the formula ------------------------------------------------------------------------------------------
def reference_np(xy, archive, ks):
    """Trajectories of length 1: euclidean_distance(x, y) = sqrt(a**2 + b**2) with a = ||x - y|| (numpy's norm: the root of a dot product) and
    b = the norm of an empty remainder, 0.0; the novelty is the mean of the k smallest, taken through argsort.  -> {k: float64 [n]}"""
    xy = np.asarray(xy, np.float32).astype(np.float64).reshape(-1, 2); archive = np.asarray(archive, np.float32).astype(np.float64).reshape(-1, 2)
    out = {k: [] for k in ks}
    for nov in xy:
        distances = []
        for point in archive:
            a = np.linalg.norm(point.reshape(1, 2) - nov.reshape(1, 2))
            b = np.linalg.norm(np.zeros((0, 2)))
            distances.append(np.sqrt(a ** 2 + b ** 2))
        distances = np.array(distances)
        for k in ks:
            out[k].append(distances[distances.argsort()[:k]].mean())
    return {k: np.array(v, np.float64) for k, v in out.items()}


# The bound between contract() and reference_np() on finite inputs, u = 2**-53, to first order in u:
#   one distance.  dx and dy are double differences of the points' coordinates, formed by the same operation on both sides: the SAME doubles.
#   Let D = sqrt(dx^2 + dy^2) exactly.  Ours: s = fl(fl(dx*dx) + fl(dy*dy)) is
#   within 2u of dx^2 + dy^2 (one product rounding that matters per term, one for the sum), its root within 1u of D, and the root's own
#   rounding adds 1u: 2u.  numpy's norm is sqrt(dot): the dot may fuse one product (one rounding fewer), never more roundings than ours: 2u.
#   The reference then squares (1u on a^2), adds an exact 0, and takes a root (halves that 1u, adds 1u): 1.5u more, 3.5u in all.
#   |ours - reference's| <= (2 + 3.5) u D = 5.5u relative.
#   order.  The i-th smallest of a list moves by no more than the largest change of any entry, so the i-th distance of one side is within
#   5.5u of the i-th of the other, whatever the two argsorts did with near-ties.
#   the sum.  kk non-negative terms added in any order: (kk - 1) u relative per side, 2 (kk - 1) u between them (numpy's pairwise mean included).
#   the division.  1u per side: 2u.
#   Together (5.5 + 2 (kk - 1) + 2) u = (2 kk + 5.5) u; rounded up to (2 kk + 6) u, which also covers the second-order terms
#   (below (2 kk + 6)^2 u^2 < 1e-12 u).
# Measured (tests/test_maze_novelty_cpu.py prints it): worst 4.36 u over the 5400 novelties of reference_cases() (the bound: 8 u at kk = 1, 70 u at kk = 32);
# 1365 of them differ from numpy in the last bits.
def reference_bound(kk):
    return (2 * kk + 6) * 2.0 ** -53


REFERENCE_KS = (1, 10, 32)


@functools.lru_cache(maxsize=None)
def reference_cases():
    """(xy [9][2], archive): archives of 1 .. 200 points in [0, 300)^2, each scored at k in REFERENCE_KS: 5400 novelties, none set aside"""
    rs = np.random.RandomState(2024)
    cases = []
    for narch in range(1, 201):
        archive = rs.uniform(0, 300, (narch, 2)).astype(np.float32)
        xy = rs.uniform(0, 300, (9, 2)).astype(np.float32)
        xy[0] = archive[rs.randint(narch)]                      # one member on an archive point
        cases.append((xy, archive))
    return cases


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def members():
    """9 members in the maze's coordinate range; the first sits on archive slot 0 of every sized archive (d = 0)"""
    xy = np.random.RandomState(7).uniform(0, 300, (9, 2)).astype(np.float32)
    xy[0] = sized_archive(SIZES[-1])[0]
    return xy


@functools.lru_cache(maxsize=None)
def sized_archive(narch):
    """the first narch points of ONE stream (so archives nest), half of them on a grid of 8: distances tie across slots and lanes"""
    rs = np.random.RandomState(11)
    pts = rs.uniform(0, 300, (SIZES[-1], 2)).astype(np.float32)
    grid = rs.rand(SIZES[-1]) < 0.5
    pts[grid] = np.round(pts[grid] / 8) * 8
    return pts[:narch].copy()


def lattice():
    return np.array([(x, y) for x in range(-3, 4) for y in range(-3, 4)], np.float32)


@functools.lru_cache(maxsize=None)
def edge_cases():
    """name -> (xy, archive, tuple of k)"""
    rs = np.random.RandomState(13)
    f = lambda *rows: np.array(rows, np.float32).reshape(-1, 2)
    some = rs.uniform(0, 300, (12, 2)).astype(np.float32)
    nan12 = some.copy(); nan12[2] = (NAN, 5.0); nan12[7] = (5.0, NAN); nan12[9] = (NAN, NAN)
    nan200 = rs.uniform(0, 300, (200, 2)).astype(np.float32)                     # a NaN early in a lane's walk, numbers after it in the same lane
    for s in (3, 67, 70, 131, 199):
        nan200[s] = (NAN, 1.0)
    mostly_nan = np.full((70, 2), NAN, np.float32); mostly_nan[[5, 64, 69]] = f((1, 1), (2, 2), (1, 1))
    dup = np.repeat(f((10, 10), (20, 5), (10, 10)), 30, axis=0)                  # 90 points, three distinct, exact ties in every lane
    return {
        "k_above_narch": (f((0, 0), (3, 4)), f((3, 4), (6, 8), (0, 1)), (4, 10, 32)),
        "member_on_a_point": (some[[4]], some, (1, 2, 12)),
        "duplicates": (f((10, 10), (0, 0), (20, 5)), dup, (1, 2, 10, 31, 32)),
        "lattice": (f((0, 0), (0.5, 0.5)), lattice(), (1, 2, 4, 5, 8, 9, 10, 12, 13, 32)),   # four- and eight-way exact ties around the origin
        "tiny_and_huge": (f((0, 0), (1e-30, -1e-30), (1e30, 1e30), (1, 1)), f((1e-30, 0), (0, 1e-30), (1e30, -1e30), (-1e30, 1e30), (3e38, 3e38), (1e-38, 1e-45), (2, 2)), (1, 2, 3, 7)),
        "inf_in_archive": (some[:3], np.concatenate([some[:5], f((INF, 0), (0, -INF), (INF, INF))]), (1, 5, 6, 8)),
        "inf_member": (f((INF, 0), (-INF, INF), (1, 1)), np.concatenate([some[:4], f((INF, 0), (-INF, 3))]), (1, 4, 6)),   # inf - inf: NaN distances
        "nan_member": (f((NAN, 1), (1, NAN), (NAN, NAN), (1, 1)), some, (1, 10, 12)),
        "nan_archive_short_and_reached": (some[:4], nan12, (1, 5, 9, 10, 11, 12, 32)),   # nine numbers: kk = 9 stops at the NaNs, kk = 10 takes the first
        "nan_in_a_lane_before_numbers": (some[:5], nan200, (1, 10, 32)),
        "mostly_nan": (f((0, 0), (1, 1)), mostly_nan, (1, 3, 4, 10, 32)),                # kk reaches NaNs in many lanes: they sort by slot
    }


def same(a, b):
    return M.same_nan(np.asarray(a, np.float64), np.asarray(b, np.float64))


# ---- dne_maze_novelty_host behind the Engine surface -------------------------------------------------------------------------------------------
class MazeNoveltyHostEngine(M.MazeHostEngine):
    """MazeHostEngine plus what dne_hip/nses_gpu.py asks of a KIND_MAZE engine: the archive of (x, y) points and maze_novelty, through
    dne_maze_novelty_host (the same header compiled for the CPU)."""

    def __init__(self, max_members=64, **kw):
        super().__init__(max_members=max_members, **kw)
        self._arch = np.zeros((0, 2), np.float32)
        self._last_n = 0

    def _run(self, thetas, tslimit):
        out = super()._run(thetas, tslimit)
        self._last_n = len(thetas)
        return out

    def _points(self, call, xy, n):
        from dne_hip import _lib
        if xy is not None:
            return np.asarray(xy, np.float32).reshape(-1, 2)
        n = self._last_n if n is None else int(n)
        if n < 1 or n > self._last_n:
            raise _lib.DneError("%s: %d members asked for, the last evaluation ran %d" % (call, n, self._last_n))
        return self._xy[:n].copy()

    def maze_archive_append(self, xy=None, n=None):
        self._arch = np.concatenate([self._arch, self._points("maze_archive_append", xy, n)])

    def maze_archive_clear(self):
        self._arch = np.zeros((0, 2), np.float32)

    def maze_archive_size(self):
        return int(self._arch.shape[0])

    def maze_archive(self):
        return self._arch.copy()

    def maze_novelty(self, k, xy=None, n=None):
        from dne_hip import _lib
        if not 1 <= int(k) <= KMAX:
            raise _lib.DneError("maze_novelty: k = %d outside 1..%d" % (k, KMAX))
        if not len(self._arch):
            raise _lib.DneError("maze_novelty: the archive is empty")
        return _lib.maze_novelty_host(self._points("maze_novelty", xy, n), self._arch, k)
