"""GPU: GA-NS on the hard maze on a DNE_KIND_MAZE engine, BIT FOR BIT.  k_maze_novelty_pool (csrc/maze_novelty.h: one wave per member, the
archive and then the population through LDS tiles, the member's own combined slot passed over) against dne_maze_novelty_pool_host on the
inputs of tests/test_maze_gans_cpu.py, in the host-xy form and in the NULL form after a real maze_ga_eval; k_maze_archive_gather; what
the two leave alone; every refusal with the archive read back; and dne_hip/ga_gpu.py's GA-NS loop on this engine against the same loop on
MazeGaNsHostEngine."""
import numpy as np
import pytest

import maze_ga_support as G
import maze_gans_support as S
import maze_support as M

pytestmark = pytest.mark.gpu

ARCHIVES = (0, 1, 63, 64, 65, 1020, 1024, 1025)   # with 9 members: the population across the tile boundary (1020), from one on (1024), behind a lone archive point (1025)
SLOT0, SLOT1 = 11, 22


def slot_theta(seed):
    return np.random.RandomState(seed).randn(S.P).astype(np.float32)


def fresh(max_members=16, prepared=True):
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_MAZE, 2, max_members=max_members)
    if prepared:
        e.noise_upload(G.noise())
        e.maze_set_walls(*M.fixture_maze())
        e.maze_ga_set_init_scale(G.scale_by())
    return e


@pytest.fixture(scope="module")
def eng():
    e = fresh()
    e.set_theta(slot_theta(SLOT0), 0)
    e.set_theta(slot_theta(SLOT1), 1)
    yield e
    assert np.array_equal(M.bits(e.get_theta(0)), M.bits(slot_theta(SLOT0))) and np.array_equal(M.bits(e.get_theta(1)), M.bits(slot_theta(SLOT1)))
    assert e.check_redzones() == 0
    e.close()


def load(eng, archive):
    eng.maze_archive_clear()
    if len(archive):
        eng.maze_archive_append(archive)
    assert eng.maze_archive_size() == len(archive)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(M.bits(a), M.bits(b))


def roots(n, seed=0):
    """n root descriptors"""
    idx = np.random.RandomState(70 + seed).randint(0, G.noise().size - S.P + 1, size=n).astype(np.int64)
    return np.full(n, -1, np.int32), idx, np.zeros(n, np.float32)


# ---- the kernel against the host twin -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", ARCHIVES)
def test_kernel_equals_host_on_every_shape(eng, A):
    from dne_hip import _lib
    assert set(ARCHIVES) <= set(S.ARCHIVES)
    archive = S.archive(A)
    load(eng, archive)
    for n in S.COUNTS:
        if A + n - 1 < 1:
            continue
        for k in S.KS:
            want = _lib.maze_novelty_pool_host(S.members()[:n], archive, k)
            got = eng.maze_novelty_pool(k, xy=S.members()[:n])
            assert got.dtype == np.float64 and S.same(got, want), (A, n, k, got, want)
    assert eng.maze_novelty_last_ms() > 0 and eng.check_redzones() == 0


@pytest.mark.parametrize("name", sorted(S.edge_cases()))
def test_kernel_equals_host_on_the_edge_inputs(eng, name):
    from dne_hip import _lib
    xy, archive, ks = S.edge_cases()[name]
    load(eng, archive)
    for k in ks:
        for n in sorted(set(min(n, len(xy)) for n in S.COUNTS)):
            if len(archive) + n - 1 < 1:
                continue
            assert S.same(eng.maze_novelty_pool(k, xy=xy[:n]), _lib.maze_novelty_pool_host(xy[:n], archive, k)), (name, k, n)
    assert eng.check_redzones() == 0


def test_null_form_scores_the_last_evaluation_where_the_rollout_left_it(eng):
    from dne_hip import _lib
    eng.maze_ga_eval(*roots(9))
    xy = eng.maze_final_state(9)
    assert len(np.unique(xy, axis=0)) > 5
    for A in (0, 65, 1020, 1025):
        archive = S.archive(A)
        load(eng, archive)
        for k in S.KS:
            want = _lib.maze_novelty_pool_host(xy, archive, k)
            assert S.same(eng.maze_novelty_pool(k), want) and S.same(eng.maze_novelty_pool(k, xy=xy), want), (A, k)
            for n in S.COUNTS:                                              # the first n members are the whole population then
                if A + n - 1 >= 1:
                    assert S.same(eng.maze_novelty_pool(k, n=n), _lib.maze_novelty_pool_host(xy[:n], archive, k)), (A, k, n)
    assert same_bits(eng.maze_final_state(9), xy) and eng.check_redzones() == 0


# ---- the gather ---------------------------------------------------------------------------------------------------------------------------------------
def test_gather_appends_members_by_index(eng):
    from dne_hip import _lib
    eng.maze_ga_eval(*roots(9, seed=1))
    xy = eng.maze_final_state(9)
    base = S.archive(3)
    for members in (list(range(9)), list(range(8, -1, -1)), [4, 4, 0, 8, 4], [7], [0], [8]):
        load(eng, base)
        eng.maze_archive_append_members(members)
        want = np.concatenate([base, xy[members]])
        assert same_bits(eng.maze_archive(), want), members
        assert S.same(eng.maze_novelty_pool(2), _lib.maze_novelty_pool_host(xy, want, 2))          # a scoring call sees the new points
    eng.maze_archive_clear()
    eng.maze_archive_append_members([2, 5])                                                        # onto an empty archive
    assert same_bits(eng.maze_archive(), xy[[2, 5]]) and eng.check_redzones() == 0


def test_gather_across_two_reallocations_of_the_archive():
    from dne_hip import _lib
    cap0 = _lib.MAZE_ARCHIVE_CAP0
    e = fresh(max_members=9)                                                                       # an archive that has never been allocated
    try:
        e.maze_ga_eval(*roots(9, seed=2))
        xy = e.maze_final_state(9)
        rs = np.random.RandomState(5)
        want = np.zeros((0, 2), np.float32)
        crossed = set()
        while len(want) <= 2 * cap0 + 9:
            members = rs.randint(0, 9, size=int(rs.randint(1, 10)))
            before = len(want)
            e.maze_archive_append_members(members)
            want = np.concatenate([want, xy[members]])
            crossed |= {c for c in (cap0, 2 * cap0) if before <= c < len(want)}
            if before <= cap0 < len(want) or before <= 2 * cap0 < len(want) or before == 0:
                assert same_bits(e.maze_archive(), want), len(want)
                assert S.same(e.maze_novelty_pool(25), _lib.maze_novelty_pool_host(xy, want, 25)), len(want)
        assert crossed == {cap0, 2 * cap0} and same_bits(e.maze_archive(), want) and e.check_redzones() == 0
    finally:
        e.close()


# ---- what the two calls leave alone ------------------------------------------------------------------------------------------------------------------
def test_no_side_effects(eng):
    from dne_hip import _lib
    bank_of = lambda: np.stack([eng.maze_ga_get_parent(j) for j in range(eng.maze_ga_parents())])
    eng.maze_ga_build(G.bank_genomes(3))
    bank = bank_of()
    members = (np.array([0, 1, 1], np.int32), np.array([5, 77, 0], np.int64), np.array([0.02, -0.02, 0.0], np.float32))
    eng.set_members(*members)
    episodes = eng.eval_members(3, 400, np.zeros(3, np.uint32))
    eng.maze_ga_eval(*G.descriptors(3, 9, seed=2))
    xy = eng.maze_final_state(9)
    archive = S.archive(65)
    load(eng, archive)
    before = eng.maze_novelty(25)
    assert S.same(before, _lib.maze_novelty_host(xy, archive, 25))
    pool = eng.maze_novelty_pool(25)
    assert S.same(pool, _lib.maze_novelty_pool_host(xy, archive, 25)) and not S.same(pool, before)
    assert S.same(eng.maze_novelty(25), before) and same_bits(eng.maze_archive(), archive)          # dne_maze_novelty gives what it gave
    eng.maze_archive_append_members([1, 3])
    assert S.same(eng.maze_novelty(25, xy=xy), _lib.maze_novelty_host(xy, np.concatenate([archive, xy[[1, 3]]]), 25))
    assert same_bits(eng.maze_final_state(9), xy) and same_bits(bank_of(), bank)
    for slot, seed in ((0, SLOT0), (1, SLOT1)):
        assert same_bits(eng.get_theta(slot), slot_theta(seed))
    again = eng.eval_members(3, 400, np.zeros(3, np.uint32))                                       # dne_set_members' members are their own
    assert all(np.array_equal(a, b) for a, b in zip(episodes, again)) and eng.check_redzones() == 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_archive_as_it_was(eng):
    from dne_hip import _lib
    one, two = np.zeros((1, 2), np.float32), np.zeros((2, 2), np.float32)
    eng.maze_ga_eval(*roots(4, seed=3))                                                           # the last evaluation ran 4 members
    eng.maze_archive_clear()
    with pytest.raises(_lib.DneError, match="dne_maze_novelty_pool: the pool is empty"):
        eng.maze_novelty_pool(1, xy=one)
    with pytest.raises(_lib.DneError, match="dne_maze_novelty_pool: the pool is empty"):
        eng.maze_novelty_pool(1, n=1)
    assert eng.maze_archive_size() == 0
    archive = S.archive(9)
    load(eng, archive)
    bad = {
        "dne_maze_novelty_pool: k = 0": lambda: eng.maze_novelty_pool(0, xy=two),
        "dne_maze_novelty_pool: k = -3": lambda: eng.maze_novelty_pool(-3, xy=two),
        "dne_maze_novelty_pool: k = 33.*DNE_MAZE_NOVELTY_KMAX = 32": lambda: eng.maze_novelty_pool(33, xy=two),
        "dne_maze_novelty_pool: n = 0": lambda: eng.maze_novelty_pool(1, xy=one[:0]),
        "dne_maze_novelty_pool: n = 0,": lambda: eng.maze_novelty_pool(1, n=0),
        "dne_maze_novelty_pool: 5 members asked for, the last evaluation ran 4": lambda: eng.maze_novelty_pool(1, n=5),
        "dne_maze_archive_append_members: count = 0": lambda: eng.maze_archive_append_members([]),
        "dne_maze_archive_append_members: index 1 is member -1, the last evaluation ran 4": lambda: eng.maze_archive_append_members([0, -1]),
        "dne_maze_archive_append_members: index 2 is member 4, the last evaluation ran 4": lambda: eng.maze_archive_append_members([0, 3, 4]),
    }
    for text, call in bad.items():
        with pytest.raises(_lib.DneError, match=text):
            call()
        assert eng.maze_archive_size() == 9 and same_bits(eng.maze_archive(), archive), text       # a refused call leaves the archive as it was
    assert S.same(eng.maze_novelty_pool(2, n=4), _lib.maze_novelty_pool_host(eng.maze_final_state(4), archive, 2))
    e = fresh(max_members=4, prepared=False)                                                       # nothing has been evaluated
    try:
        e.maze_archive_append(one)
        for call in (lambda: e.maze_novelty_pool(1), lambda: e.maze_novelty_pool(1, n=1), lambda: e.maze_archive_append_members([0])):
            with pytest.raises(_lib.DneError, match="last evaluation|n = 0"):
                call()
        assert e.maze_archive_size() == 1
    finally:
        e.close()
    other = _lib.Engine(_lib.KIND_GA, 18, max_members=4)
    try:
        for name, call in (("dne_maze_novelty_pool", lambda: other.maze_novelty_pool(1, xy=two)),
                           ("dne_maze_archive_append_members", lambda: other.maze_archive_append_members([0]))):
            with pytest.raises(_lib.DneError, match=name + r" needs a DNE_KIND_MAZE engine \(this one: kind 1\)"):
                call()
    finally:
        other.close()
    assert eng.check_redzones() == 0


# ---- the driver --------------------------------------------------------------------------------------------------------------------------------------------
def _table():
    from dne_hip import es
    t = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    t.noise, t._engines = G.noise(), []
    return t


def _exp(ns=None, **over):
    exp = {"game": "maze", "model": "SimpleClassifier", "population_size": 10, "selection_threshold": 3, "validation_threshold": 2,
           "num_validation_episodes": 2, "num_test_episodes": 2, "episode_cutoff_mode": 400, "mutation_power": 0.005, "timesteps": 10 ** 9,
           "maze_file": M.MAZE_FILE, "novelty_search": {"k": 3, "archive_prob": 0.3}}
    exp.update(over)
    exp["novelty_search"] = dict(exp["novelty_search"], **(ns or {}))
    return exp


CONFIGS = {"prob_0.3": dict(), "prob_1_k_25": dict(ns={"archive_prob": 1.0, "k": 25}), "no_parents_prob_0": dict(selection_threshold=0, ns={"archive_prob": 0.0})}


def _same_run(a, b):
    (ta, va, sa), (tb, vb, sb) = a, b
    ok = (ta, va) == (tb, vb) and sa.it == sb.it and [o.seeds for o in sa.population] == [o.seeds for o in sb.population]
    ok = ok and [o.rewards for o in sa.population] == [o.rewards for o in sb.population] and sa.elite.seeds == sb.elite.seeds
    ok = ok and [o.novelty for o in sa.population] == [o.novelty for o in sb.population] and same_bits(sa.archive, sb.archive)
    return ok and (sa.curr_solution, sa.timesteps_so_far, sa.num_frames) == (sb.curr_solution, sb.timesteps_so_far, sb.num_frames)


def _recording(engine):
    """every pool score the engine returns, kept"""
    seen, inner = [], engine.maze_novelty_pool

    def maze_novelty_pool(k, xy=None, n=None):
        seen.append(inner(k, xy=xy, n=n))
        return seen[-1]

    engine.maze_novelty_pool = maze_novelty_pool
    return seen


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_driver_on_the_hip_engine_equals_the_host_engine(oracle, tmp_path, config):
    from dne_hip import ga_gpu
    over = CONFIGS[config]
    hip, host = fresh(max_members=10, prepared=False), S.MazeGaNsHostEngine(max_members=10)
    try:
        hip.set_theta(slot_theta(SLOT0), 0)
        seen = _recording(hip)
        for it in (2, 4):                                                                          # two generations, then two more resumed, on each side
            a = ga_gpu.main(str(tmp_path / "hip"), engine=hip, noise=_table(), seed=4, max_iters=2, **_exp(**over))
            b = ga_gpu.main(str(tmp_path / "host"), engine=host, noise=_table(), seed=4, max_iters=2, **_exp(**over))
            assert a[2].it == it and a[2].algo == "ga_ns" and _same_run(a, b)
            assert same_bits(hip.maze_archive(), host.maze_archive()) and hip.maze_ga_parents() == host.maze_ga_parents()
            assert all(same_bits(hip.maze_ga_get_parent(j), host.bank[j]) for j in range(hip.maze_ga_parents()))
            assert len(seen) == it and all(S.same(x, y) for x, y in zip(seen, host.novelties))
        assert same_bits(hip.get_theta(0), slot_theta(SLOT0)) and hip.check_redzones() == 0
    finally:
        hip.close()


def test_driver_builds_its_own_engine(oracle, tmp_path):
    from dne_hip import ga_gpu
    a = ga_gpu.main(str(tmp_path / "own"), noise=_table(), seed=4, max_iters=3, **_exp())
    b = ga_gpu.main(str(tmp_path / "host"), engine=S.MazeGaNsHostEngine(max_members=10), noise=_table(), seed=4, max_iters=3, **_exp())
    assert a[2].it == 3 and _same_run(a, b) and len(a[2].archive) > 0
