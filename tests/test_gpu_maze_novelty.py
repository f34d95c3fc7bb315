"""GPU: k_maze_novelty (csrc/maze_novelty.h: one wave per member, the archive through LDS tiles, each lane's neighbours sorted in registers)
on a DNE_KIND_MAZE engine against dne_maze_novelty_host -- the same header compiled for the CPU -- BIT FOR BIT, on the inputs of
tests/test_maze_novelty_cpu.py and member counts 1, 3, 4, 5, 9; the device-to-device forms (xy=None); the archive across its reallocation;
the refusals; and dne_hip/nses_gpu.py on this engine against the same driver on MazeNoveltyHostEngine."""
import functools

import numpy as np
import pytest

import maze_novelty_support as S
import maze_support as M

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def noise():
    return M.maze_noise()


@pytest.fixture(scope="module")
def eng():
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_MAZE, 2, max_members=16)
    e.noise_upload(noise())
    e.set_theta(M.theta0(noise()))
    e.maze_set_walls(*M.fixture_maze())
    yield e
    assert e.check_redzones() == 0
    e.close()


def load(eng, archive):
    eng.maze_archive_clear()
    eng.maze_archive_append(archive)
    assert eng.maze_archive_size() == len(archive)


@pytest.mark.parametrize("narch", S.SIZES)
def test_kernel_equals_host_on_every_archive_size(eng, narch):
    from dne_hip import _lib
    archive = S.sized_archive(narch)
    load(eng, archive)
    assert np.array_equal(M.bits(eng.maze_archive()), M.bits(archive))
    for k in S.KS:
        want = _lib.maze_novelty_host(S.members(), archive, k)
        for n in S.COUNTS:
            got = eng.maze_novelty(k, xy=S.members()[:n])
            assert got.dtype == np.float64 and S.same(got, want[:n]), (narch, k, n, got, want[:n])
    assert eng.check_redzones() == 0


@pytest.mark.parametrize("name", sorted(S.edge_cases()))
def test_kernel_equals_host_on_the_edge_inputs(eng, name):
    from dne_hip import _lib
    xy, archive, ks = S.edge_cases()[name]
    load(eng, archive)
    back = eng.maze_archive()
    assert M.same_nan(back, archive)
    for k in ks:
        want = _lib.maze_novelty_host(xy, archive, k)
        for n in sorted(set(min(n, len(xy)) for n in S.COUNTS)):
            assert S.same(eng.maze_novelty(k, xy=xy[:n]), want[:n]), (name, k, n)
    assert eng.check_redzones() == 0


def test_device_to_device_forms(eng):
    """xy=None: the last evaluation's final positions are scored and appended where k_maze_rollout left them"""
    from dne_hip import _lib
    load(eng, S.sized_archive(65))
    idx = np.random.RandomState(3).randint(0, noise().size - M.P + 1, size=5).astype(np.int64)
    eng.es_eval(idx, 0.02, 400, np.zeros(10, np.uint32))
    xy = eng.maze_final_state(10)
    assert len(np.unique(xy, axis=0)) > 5
    for k in (1, 10, 32):
        want = _lib.maze_novelty_host(xy, S.sized_archive(65), k)
        assert S.same(eng.maze_novelty(k), want) and S.same(eng.maze_novelty(k, xy=xy), want)
        for n in (1, 3, 4, 5, 9):
            assert S.same(eng.maze_novelty(k, n=n), want[:n])
    for n in (1, 3, 10):
        eng.maze_archive_clear()
        eng.maze_archive_append(n=n)
        a = eng.maze_archive()
        eng.maze_archive_clear()
        eng.maze_archive_append(xy[:n])
        assert a.shape == (n, 2) and np.array_equal(M.bits(a), M.bits(eng.maze_archive())) and np.array_equal(M.bits(a), M.bits(xy[:n]))
    eng.maze_archive_clear()
    eng.maze_archive_append()                                        # without n: every member of the last evaluation
    assert np.array_equal(M.bits(eng.maze_archive()), M.bits(xy))
    assert eng.check_redzones() == 0


def test_archive_grows_across_its_reallocation(eng):
    from dne_hip import _lib
    cap0 = _lib.MAZE_ARCHIVE_CAP0
    pts = S.sized_archive(2 * cap0 + 3)
    fresh = _lib.Engine(_lib.KIND_MAZE, 2, max_members=4)            # an archive that has never been allocated
    try:
        assert fresh.maze_archive_size() == 0 and fresh.maze_archive().shape == (0, 2)
        for i, p in enumerate(pts):
            fresh.maze_archive_append(p)
            if i + 1 in (1, cap0 - 1, cap0, cap0 + 1, 2 * cap0, 2 * cap0 + 1, len(pts)):    # before and after each reallocation
                assert fresh.maze_archive_size() == i + 1
                assert np.array_equal(M.bits(fresh.maze_archive()), M.bits(pts[:i + 1]))
                assert S.same(fresh.maze_novelty(10, xy=S.members()), _lib.maze_novelty_host(S.members(), pts[:i + 1], 10)), i
        fresh.maze_archive_append(pts)                               # many at once, past the capacity again
        assert np.array_equal(M.bits(fresh.maze_archive()), M.bits(np.concatenate([pts, pts])))
        assert fresh.check_redzones() == 0
    finally:
        fresh.close()


def test_refusals(eng):
    from dne_hip import _lib
    one = np.zeros((1, 2), np.float32)
    eng.maze_archive_clear()
    with pytest.raises(_lib.DneError, match="dne_maze_novelty: the archive is empty"):
        eng.maze_novelty(1, xy=one)
    archive = S.sized_archive(9)
    load(eng, archive)
    eng.es_eval(np.zeros(2, np.int64), 0.0, 7, np.zeros(4, np.uint32))          # the last evaluation ran 4 members
    bad = {
        "k = 0": lambda: eng.maze_novelty(0, xy=one),
        "k = -3": lambda: eng.maze_novelty(-3, xy=one),
        "k = 33.*DNE_MAZE_NOVELTY_KMAX = 32": lambda: eng.maze_novelty(33, xy=one),
        "dne_maze_novelty: n = 0": lambda: eng.maze_novelty(1, xy=one[:0]),
        "dne_maze_novelty: 5 members asked for, the last evaluation ran 4": lambda: eng.maze_novelty(1, n=5),
        "dne_maze_novelty: n = 0,": lambda: eng.maze_novelty(1, n=0),
        "dne_maze_archive_append: n = 0": lambda: eng.maze_archive_append(one[:0]),
        "dne_maze_archive_append: 5 members asked for, the last evaluation ran 4": lambda: eng.maze_archive_append(n=5),
        "dne_maze_archive_get: room for 8 points, the archive holds 9": lambda: eng._ck(eng.lib.dne_maze_archive_get(eng.h, None, 8)),
    }
    for text, call in bad.items():
        with pytest.raises(_lib.DneError, match=text):
            call()
        assert eng.maze_archive_size() == 9 and np.array_equal(M.bits(eng.maze_archive()), M.bits(archive)), text   # a refused call leaves the archive as it was
    assert S.same(eng.maze_novelty(2, n=4), _lib.maze_novelty_host(eng.maze_final_state(4), archive, 2))
    # a fresh engine: nothing has been evaluated
    fresh = _lib.Engine(_lib.KIND_MAZE, 2, max_members=4)
    try:
        fresh.maze_archive_append(one)
        for call in (lambda: fresh.maze_novelty(1), lambda: fresh.maze_novelty(1, n=1), lambda: fresh.maze_archive_append(n=1), lambda: fresh.maze_archive_append()):
            with pytest.raises(_lib.DneError, match="last evaluation|n = 0"):
                call()
        assert fresh.maze_archive_size() == 1
    finally:
        fresh.close()
    # every engine call on an engine of another kind, by name
    other = _lib.Engine(_lib.KIND_GA, 18, max_members=4)
    try:
        calls = {
            "dne_maze_archive_append": lambda: other.maze_archive_append(one),
            "dne_maze_archive_clear": lambda: other.maze_archive_clear(),
            "dne_maze_archive_size": lambda: other.maze_archive_size(),
            "dne_maze_archive_get": lambda: other._ck(other.lib.dne_maze_archive_get(other.h, None, 0)),
            "dne_maze_novelty": lambda: other.maze_novelty(1, xy=one),
        }
        for name, call in calls.items():
            with pytest.raises(_lib.DneError, match=name + r" needs a DNE_KIND_MAZE engine \(this one: kind 1\)"):
                call()
    finally:
        other.close()
    assert eng.check_redzones() == 0


@pytest.mark.parametrize("algo_type", ("ns", "nsr"))
@pytest.mark.parametrize("method", ("round_robin", "novelty_prob"))
def test_driver_on_the_hip_engine_equals_the_host_function_engine(oracle, tmp_path, algo_type, method):
    from dne_hip import _lib, es, nses_gpu
    exp = {"game": "maze", "model": "SimpleClassifier", "algo_type": algo_type, "population_size": 8, "timesteps": 10 ** 9,
           "novelty_search": {"k": 2, "population_size": 3, "num_rollouts": 1, "selection_method": method},
           "episode_cutoff_mode": "env_default", "return_proc_mode": "centered_sign_rank", "l2coeff": 0.005, "mutation_power": 0.02,
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}, "maze_file": M.MAZE_FILE}

    def table():
        t = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
        t.noise, t._engines = noise(), []
        return t

    hip = _lib.Engine(_lib.KIND_MAZE, 2, max_members=8)
    try:
        a = nses_gpu.main(str(tmp_path / "hip"), engine=hip, noise=table(), seed=3, max_iters=3, **exp)
        assert hip.check_redzones() == 0 and np.array_equal(M.bits(hip.maze_archive()), M.bits(a.archive))
    finally:
        hip.close()
    b = nses_gpu.main(str(tmp_path / "host"), engine=S.MazeNoveltyHostEngine(max_members=8), noise=table(), seed=3, max_iters=3, **exp)
    assert a.it == b.it == 3 and a.parents == b.parents and a.curr_parent == b.curr_parent and a.archive.shape == (6, 2)
    assert np.array_equal(M.bits(a.archive), M.bits(b.archive)) and a.novelty_log == b.novelty_log
    for x, y in zip(a.thetas, b.thetas):
        assert np.array_equal(M.bits(x), M.bits(y))
    for x, y in zip(a.optimizers, b.optimizers):
        assert np.array_equal(M.bits(x[0]), M.bits(y[0])) and np.array_equal(M.bits(x[1]), M.bits(y[1])) and x[2] == y[2]
