"""GPU: k_maze_rollout (csrc/maze.h: whole hard-maze episodes in one launch, 16 lanes per member, four members per wave) on a DNE_KIND_MAZE engine
against dne_maze_rollout_host -- the same header compiled for the CPU -- BIT FOR BIT: returns, sign-returns, lengths, final (x, y), the per-step
trace of chosen members, the recorded behaviour.  Member counts 1, 2, 3, 4, 5, 64, 67 (one row, a wave's four members, a wave plus one, partial
last waves), 1 and 33 pairs through dne_es_eval, timestep limits 1, 7, 399, 400, mazes of 13 (the fixture), 1, 17 and 64 walls; then one ES update,
the es_gpu.py driver on this engine against the driver on the host-function engine, the wire records, and the kind's refusals.

The member set (67 members): theta_0 +- sigma * eps at sigma 0.02 and at sigma 1.0 (outputs saturate the clamps), power-0 members, members on a
second base slot, and hand-made thetas that drive straight into a wall and that spin in place."""
import functools

import numpy as np
import pytest

import maze_support as M

pytestmark = pytest.mark.gpu
COUNTS = (1, 2, 3, 4, 5, 64, 67)
LIMITS = (1, 7, 399, 400)
WALLS = (13, 1, 17, 64)
NMEM = 67
TRACED = (0, 3, 4, 5, 63, 66)            # first row, last row of the first wave, first row of the second, ..., the lone member of the last wave


@functools.lru_cache(maxsize=None)
def noise():
    return M.maze_noise()


@functools.lru_cache(maxsize=None)
def bases():
    """base slots: 0 = theta_0, 1 = another start, 2 = straight into a wall, 3 = spin in place"""
    return [M.theta0(noise(), 1234), M.theta0(noise(), 40_000), M.straight_into_wall_theta(), M.spin_in_place_theta()]


@functools.lru_cache(maxsize=None)
def members():
    """(slot, offset, scale) of the 67 members"""
    rs = np.random.RandomState(5)
    slot = np.zeros(NMEM, np.int32); off = rs.randint(0, noise().size - M.P + 1, size=NMEM).astype(np.int64); scale = np.zeros(NMEM, np.float32)
    for i in range(NMEM):
        kind = i % 8
        scale[i] = (0.02, -0.02, 1.0, -1.0, 0.0, 0.02, 0.0, 0.0)[kind]
        slot[i] = (0, 0, 0, 0, 0, 1, 2, 3)[kind]
    off[1] = off[0]; off[3] = off[2]                    # members (0, 1) and (2, 3) are antithetic pairs
    off[-1] = noise().size - M.P                        # the last legal slice of the table
    return slot, off, scale


@functools.lru_cache(maxsize=None)
def member_thetas():
    slot, off, scale = members()
    return np.stack([M.perturbed(bases()[slot[i]], noise(), int(off[i]), scale[i]) for i in range(NMEM)])


@functools.lru_cache(maxsize=None)
def maze(nw):
    return M.fixture_maze() if nw == 13 else M.synthetic_maze(nw)


@functools.lru_cache(maxsize=None)
def host(nw, tslimit):
    """the CPU side of every comparison, once per (maze, limit): returns, lengths, final xy, trace of all 67 members"""
    from dne_hip import _lib
    header, lines = maze(nw)
    return _lib.maze_rollout_host(member_thetas(), header, lines, tslimit, want_trace=True)


@pytest.fixture(scope="module")
def eng():
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_MAZE, 2, max_members=80, record_bc=True, bc_max_steps=400)
    e.noise_upload(noise())
    for s, th in enumerate(bases()):
        e.set_theta(th, slot=s)
    yield e
    e.close()


def same(a, b):
    return np.array_equal(M.bits(a), M.bits(b))


def test_member_set_is_what_the_docstring_says():
    """held on the host function alone: the hand-made thetas do what they are for, sigma 1.0 saturates, and the episodes differ"""
    ret, ln, xy, trace = host(13, 400)
    slot, off, scale = members()
    header, _ = maze(13)
    wall, spin = np.flatnonzero(slot == 2), np.flatnonzero(slot == 3)
    assert np.all(xy[spin] == header[2:4]) and np.all(np.abs(trace[spin, -1, 15]) == 3.0)              # never moved, turning at the clamp
    assert np.all(xy[wall, 0] > header[2] + 10) and np.all(trace[wall, -1, 14] == 3.0) and same(trace[wall[0], -1, 11:13], trace[wall[0], -100, 11:13])   # pinned
    big = np.flatnonzero(np.abs(scale) == 1.0)
    assert np.any(np.abs(trace[big][:, :, 14]) == 3.0) or np.any(np.abs(trace[big][:, :, 15]) == 3.0)  # outputs beyond the clamps
    assert np.all(ln == 400) and np.all(ret < 0) and len(np.unique(ret)) > 20
    assert same(ret[4], ret[12]) and not same(ret[0], ret[1])                                          # power-0 members are theta_0 itself


@pytest.mark.parametrize("nw", WALLS)
def test_kernel_equals_host_bit_for_bit(eng, nw):
    header, lines = maze(nw)
    assert lines.shape[0] == nw
    eng.maze_set_walls(header, lines)
    slot, off, scale = members()
    for n in COUNTS:
        eng.set_members(slot[:n], off[:n], scale[:n])
        for tslimit in LIMITS:
            hret, hln, hxy, htrace = host(nw, tslimit)
            ret, sg, ln = eng.eval_members(n, tslimit, np.zeros(n, np.uint32))
            assert same(ret, hret[:n]) and np.array_equal(ln, hln[:n]) and same(sg, np.sign(hret[:n])), (nw, n, tslimit)
            assert same(eng.maze_final_state(n), hxy[:n]), (nw, n, tslimit)
            assert np.all(ln == tslimit) and (tslimit == 400 or np.all(ret == 0))
            for m in TRACED:
                if m < n and (n in (5, 67) or tslimit == 7):
                    assert same(eng.maze_debug_trace(m, tslimit), htrace[m]), (nw, n, tslimit, m)
            assert same(eng.maze_final_state(n), hxy[:n])            # the trace launches left the evaluation's results alone
        assert eng.check_redzones() == 0
    # behaviour: (x, y) after every step of every member = the trace's position columns; rows past a shorter episode stay zero
    eng.set_members(slot, off, scale)
    for tslimit in (400, 7):
        ret, sg, ln, bc = eng.eval_members(NMEM, tslimit, np.zeros(NMEM, np.uint32), want_bc=True)
        htrace = host(nw, tslimit)[3]
        assert bc.shape == (NMEM, 400, 2) and same(bc[:, :tslimit], htrace[:, :, 11:13]) and not np.any(bc[:, tslimit:])
    assert eng.check_redzones() == 0


@pytest.mark.parametrize("sigma", (0.02, 1.0))
def test_pairs_through_es_eval(eng, sigma):
    from dne_hip import _lib
    header, lines = maze(13)
    eng.maze_set_walls(header, lines)
    eng.set_theta(bases()[0])
    idx = np.random.RandomState(9).randint(0, noise().size - M.P + 1, size=33).astype(np.int64)
    for n in (1, 33):
        th = np.stack([M.perturbed(bases()[0], noise(), int(i), s) for i in idx[:n] for s in (sigma, -sigma)])
        for tslimit in (400, 399):
            hret, hln, hxy = _lib.maze_rollout_host(th, header, lines, tslimit)
            ret, sg, ln = eng.es_eval(idx[:n], sigma, tslimit, np.arange(2 * n, dtype=np.uint32) * 977)    # (seeds: accepted and ignored)
            assert ret.shape == (n, 2) and same(ret.reshape(-1), hret) and np.array_equal(ln.reshape(-1), hln) and same(sg.reshape(-1), np.sign(hret))
            assert same(eng.maze_final_state(2 * n), hxy)
        rec = eng.records_pack(n)                                    # the wire records of the last evaluation (tslimit 399)
        assert np.array_equal(rec["noise_idx"], idx[:n]) and same(rec["ret"], ret) and np.array_equal(rec["len"], ln) and same(rec["aux"], sg)
    assert eng.check_redzones() == 0


def test_one_es_update_equals_the_update_from_the_host_returns(eng, oracle):
    from dne_hip import _lib
    header, lines = maze(13)
    eng.maze_set_walls(header, lines)
    th0 = bases()[0]
    eng.set_theta(th0)
    eng.optimizer_reset()
    idx = np.random.RandomState(10).randint(0, noise().size - M.P + 1, size=33).astype(np.int64)
    ret, sg, ln = eng.es_eval(idx, 0.02, 400, np.zeros(66, np.uint32))
    th = np.stack([M.perturbed(th0, noise(), int(i), s) for i in idx for s in (0.02, -0.02)])
    hret = _lib.maze_rollout_host(th, header, lines, 400)[0].reshape(33, 2)
    assert same(ret, hret)
    eng.es_update(idx, ret, sg, "centered_rank", "adam", 0.005, 0.01)
    opt = oracle.Adam(th0, 0.01)
    _, want = opt.update(oracle.es_gradient(noise(), idx, hret, M.P), 0.005)
    m, v, t = eng.optimizer_get_state()
    assert same(eng.get_theta(), want) and same(m, opt.m) and same(v, opt.v) and t == 1 and not same(want, th0)
    # the same update through the gathered records
    eng.set_theta(th0); eng.optimizer_reset()
    eng.es_eval(idx, 0.02, 400, np.zeros(66, np.uint32))
    eng.records_set(eng.records_pack(33))
    eng.es_update_gathered("centered_rank", "adam", 0.005, 0.01)
    assert same(eng.get_theta(), want)
    g = eng.weighted_sum(idx[:5], np.arange(5, dtype=np.float32) - 2, 10.0)
    assert same(g, oracle.weighted_sum(noise(), idx[:5], np.arange(5, dtype=np.float32) - 2, M.P, 10.0))
    assert eng.check_redzones() == 0


def test_driver_on_the_hip_engine_equals_the_host_function_engine(oracle, tmp_path):
    from dne_hip import _lib, es, es_gpu
    exp = {"game": "maze", "model": "SimpleClassifier", "num_test_episodes": 2, "population_size": 10, "timesteps": 10 ** 9,
           "episode_cutoff_mode": "env_default", "return_proc_mode": "centered_rank", "l2coeff": 0.005, "mutation_power": 0.02,
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}, "maze_file": M.MAZE_FILE}

    def table():
        t = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
        t.noise, t._engines = noise(), []
        return t

    hip = _lib.Engine(_lib.KIND_MAZE, 2, max_members=10)
    try:
        a = es_gpu.main(str(tmp_path / "hip"), engine=hip, noise=table(), seed=3, max_iters=2, **exp)
        assert hip.check_redzones() == 0
    finally:
        hip.close()
    b = es_gpu.main(str(tmp_path / "host"), engine=M.MazeHostEngine(max_members=10), noise=table(), seed=3, max_iters=2, **exp)
    assert a.it == b.it == 2 and a.timesteps_so_far == b.timesteps_so_far == 2 * 10 * 400 and a.game == "maze"
    assert same(a.theta, b.theta) and same(a.optimizer[0], b.optimizer[0]) and same(a.optimizer[1], b.optimizer[1]) and a.optimizer[2] == 2
    # the engine the driver builds for itself when none is passed in
    c = es_gpu.main(str(tmp_path / "own"), noise=table(), seed=3, max_iters=2, **exp)
    assert same(c.theta, b.theta)


def test_refusals(eng):
    from dne_hip import _lib
    with pytest.raises(_lib.DneError, match="n_actions 18"):
        _lib.Engine(_lib.KIND_MAZE, 18, max_members=4)
    with pytest.raises(_lib.DneError, match=r"bc_final_only is not available on a DNE_KIND_MAZE engine \(kind 4\).*dne_maze_final_state"):
        _lib.Engine(_lib.KIND_MAZE, 2, max_members=4, record_bc=True, bc_max_steps=400, bc_final_only=True)
    fresh = _lib.Engine(_lib.KIND_MAZE, 2, max_members=4)
    try:
        fresh.noise_upload(noise())
        with pytest.raises(_lib.DneError, match="dne_maze_set_walls"):           # an evaluation before the walls: a clean error
            fresh.es_eval(np.zeros(1, np.int64), 0.02, 400, np.zeros(2, np.uint32))
        header, lines = maze(13)
        for n in (0, 65):
            with pytest.raises(_lib.DneError, match="1..64"):
                fresh.maze_set_walls(header, np.zeros((n, 4), np.float32))
        fresh.maze_set_walls(header, lines)
        with pytest.raises(_lib.DneError, match="max_members"):
            fresh.es_eval(np.zeros(3, np.int64), 0.02, 400, np.zeros(6, np.uint32))
        with pytest.raises(_lib.DneError, match="outside the table"):
            fresh.es_eval(np.array([noise().size - M.P + 1], np.int64), 0.02, 400, np.zeros(2, np.uint32))
        with pytest.raises(_lib.DneError, match="record_bc"):
            fresh.eval_members(1, 400, np.zeros(1, np.uint32), want_bc=True)
        with pytest.raises(_lib.DneError, match="last evaluation"):
            fresh.maze_final_state(1)
        assert fresh.check_redzones() == 0
    finally:
        fresh.close()
    one = np.zeros(1, np.uint32)
    calls = {
        "dne_ga_eval": lambda: eng.ga_eval([[1, 2]], 0.01, 10, one),
        "dne_ga_eval_powers": lambda: eng.ga_eval_powers([((1,), (2, 0.1))], 10, one),
        "dne_ga_rebuild": lambda: eng.ga_rebuild(0, [1, 2], 0.01),
        "dne_ga_rebuild_powers": lambda: eng.ga_rebuild_powers(0, ((1,), (2, 0.1))),
        "dne_ga_set_init_scale": lambda: eng.ga_set_init_scale(np.zeros(M.P, np.float32)),
        "dne_ref_pass": lambda: eng.ref_pass(1),
        "dne_set_ref_batch": lambda: eng.lib.dne_set_ref_batch(eng.h, None, 8) and eng._ck(-1),
        "dne_env_reset": lambda: eng.env_reset(one),
        "dne_env_step": lambda: eng.env_step(np.zeros(1, np.int32)),
        "dne_env_observation": lambda: eng.env_observation(1),
        "dne_env_ram": lambda: eng.env_ram(1),
        "dne_env_set_observation": lambda: eng.env_set_observation(np.zeros((1, 84, 84, 4), np.uint8)),
        "dne_env_set_ram": lambda: eng.env_set_ram(np.zeros((1, 128), np.uint8), np.zeros((1, 128), np.uint8)),
        "dne_act": lambda: eng.act(1),
        "dne_get_bn": lambda: eng.get_bn(1),
        "dne_novelty": lambda: eng.novelty([], np.zeros((1, 128), np.uint8), 1),
        "dne_novelty_batch": lambda: eng.novelty_batch([], [1], 1),
        "dne_novelty_knn": lambda: eng.novelty_knn([], 1, bcs=[np.zeros((1, 128), np.uint8)]),
    }
    for name, call in calls.items():
        with pytest.raises(_lib.DneError, match=name + r" is not available on a DNE_KIND_MAZE engine \(kind 4\)"):
            call()
    with pytest.raises(_lib.DneError, match="kind 4"):
        _lib.debug_plan(_lib.KIND_MAZE, 2, 8, 2)
    # and the maze calls on an engine of another kind
    other = _lib.Engine(_lib.KIND_GA, 18, max_members=4)
    try:
        with pytest.raises(_lib.DneError, match="DNE_KIND_MAZE"):
            other.maze_set_walls(*maze(13))
        with pytest.raises(_lib.DneError, match="DNE_KIND_MAZE"):
            other.maze_final_state(1)
        with pytest.raises(_lib.DneError, match="dne_maze_debug_math needs a DNE_KIND_MAZE engine"):
            other.maze_debug_math(0, [0.5])
    finally:
        other.close()
    assert eng.check_redzones() == 0
