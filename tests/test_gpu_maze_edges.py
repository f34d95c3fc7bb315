"""GPU: k_maze_rollout on the ground tests/golden/maze_reference_edges.npz covers on the CPU -- `disable` 1, a zero-length wall, walls at distance
exactly 8.0 and 7.99, the goal straight above / below / on the start, rays that end on wall ends -- closed loop against dne_maze_rollout_host,
BIT FOR BIT except for the payload and sign of a NaN (maze_support.same_nan).  23 members per maze (three in the last wave): constant-action
thetas, output biases NaN / +-inf / +-1e30 / denormal, weights near FLT_MAX (the fmaf chains overflow inside an episode), theta_0 +- sigma * eps.
Then the placement of one hit among 64 walls dealt over 16 lanes, one ES step whose returns tie at -500, the recording capacities, and
k_maze_math (the trigonometry outside an episode) against dne_maze_math_host on the probe's inputs."""
import functools

import numpy as np
import pytest

import maze_support as M

pytestmark = pytest.mark.gpu
LIMITS = (400, 7)
NAN, INF = np.float32(np.nan), np.float32(np.inf)
BIASES = ((0, 0), (0, 0.7), (0.7, 0), (-0.3, 0.5), (1e-40, -1e-40),                       # the recording's constant pairs
          (NAN, 0.7), (0.0, NAN), (NAN, NAN), (INF, INF), (-INF, 1e30), (-1e30, -INF), (1e30, INF), (-INF, -1e30))
NAN_MEMBERS = (5, 6, 7)                                                                    # a NaN action on every step
HUGE = 13                                                                                  # weights near FLT_MAX
NMEM = 23
TRACED = (0, 1, 3, 5, 6, 13, 19, 22)


@functools.lru_cache(maxsize=None)
def noise():
    return M.maze_noise()


@functools.lru_cache(maxsize=None)
def thetas():
    """[23][498]: 13 constant-action thetas, the huge one, theta_0, then theta_0 +- sigma * eps at sigma 0.02 and 1.0 (two pairs each)"""
    th = [M.constant_action_theta(*b) for b in BIASES]
    i = np.arange(M.P)
    huge = np.where((i + i // 16) % 2 == 0, np.float32(3e38), np.float32(-3e38)).astype(np.float32)   # signs alternate along every chain: the
    huge[M.B3:] = (0.1, 0.2)                                    # products overflow to +inf and -inf and meet as NaN inside the forward pass
    th.append(huge)
    base = M.theta0(noise())
    th.append(base)
    rs = np.random.RandomState(11)
    for sigma in (0.02, 1.0):
        for off in rs.randint(0, noise().size - M.P + 1, size=2):
            th += [M.perturbed(base, noise(), int(off), sigma), M.perturbed(base, noise(), int(off), -sigma)]
    th = np.stack(th)
    assert th.shape == (NMEM, M.P) and NMEM % 4 == 3
    return th


@functools.lru_cache(maxsize=None)
def host(name, tslimit):
    from dne_hip import _lib
    header, lines = M.edge_maze(name)
    return _lib.maze_rollout_host(thetas(), header, lines, tslimit, want_trace=True)


def upload(e, th):
    """every theta its own base slot, power 0: the members ARE the thetas, NaN and infinite parameters included"""
    for s, t in enumerate(th):
        e.set_theta(t, slot=s)
    n = len(th)
    e.set_members(np.arange(n, dtype=np.int32), np.zeros(n, np.int64), np.zeros(n, np.float32))


@pytest.fixture(scope="module")
def eng():
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_MAZE, 2, max_members=NMEM, record_bc=True, bc_max_steps=400)
    e.noise_upload(noise())
    upload(e, thetas())
    yield e
    assert e.check_redzones() == 0
    e.close()


def test_member_set_on_the_host():
    """held on the host function alone: what the members are for happens"""
    for name in M.EDGE_MAZES:
        ret, ln, xy, trace = host(name, 400)
        header, _ = M.edge_maze(name)
        assert np.all(ln == 400)
        moved = [i for i in range(NMEM) if not np.array_equal(xy[i], header[2:4])]
        if name == "zero_wall":
            assert not moved and np.all(np.isfinite(ret))                                  # every step collides: nobody moves, NaN action or not
        else:
            assert np.all(ret[list(NAN_MEMBERS)] == -500) and np.all(np.isnan(xy[list(NAN_MEMBERS)]))
            assert np.isfinite(ret[HUGE]) or ret[HUGE] == -500
        others = [i for i in range(NMEM) if i not in NAN_MEMBERS and i != HUGE]
        assert np.all(np.isfinite(trace[others])) and np.all(np.isfinite(ret[others])) and np.all(ret[others] <= 0)
        if name not in ("zero_wall", "dist_7_99", "dist_8"):                           # (where the wall ahead is not already in touch)
            assert 1 in moved and 0 not in moved and 2 not in moved                        # straight moves, still and spin stay
    # the huge theta overflows inside the forward pass: with the radar bits of this maze the hidden layers hold +inf, and -inf + inf = NaN
    from dne_hip import _lib
    h1, h2, out = _lib.maze_forward_host(thetas()[HUGE], np.array([1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1], np.float32))
    assert np.any(np.isinf(h2)) and np.all(np.isnan(out))


@pytest.mark.parametrize("name", M.EDGE_MAZES)
def test_kernel_equals_host_on_the_edge_mazes(eng, name):
    header, lines = M.edge_maze(name)
    eng.maze_set_walls(header, lines)
    for tslimit in LIMITS:
        hret, hln, hxy, htrace = host(name, tslimit)
        ret, sg, ln, bc = eng.eval_members(NMEM, tslimit, np.zeros(NMEM, np.uint32), want_bc=True)
        with np.errstate(invalid="ignore"):
            hsign = ((hret > 0).astype(np.float32) - (hret < 0).astype(np.float32))
        assert M.same_nan(ret, hret) and np.array_equal(ln, hln) and M.same_nan(sg, hsign), (name, tslimit)
        assert not np.any(np.isnan(ret)) and np.all(ln == tslimit)
        xy = eng.maze_final_state(NMEM)
        assert M.same_nan(xy, hxy), (name, tslimit)
        assert bc.shape == (NMEM, 400, 2) and M.same_nan(bc[:, :tslimit], np.ascontiguousarray(htrace[:, :, 11:13])) and not np.any(bc[:, tslimit:])
        for m in TRACED:
            assert M.same_nan(eng.maze_debug_trace(m, tslimit), htrace[m]), (name, tslimit, m)
        # the consequences, on the device's own results
        if tslimit == 400:
            if name == "zero_wall":
                assert np.all(xy == header[2:4]) and np.all(bc == header[2:4])
            else:
                nm = list(NAN_MEMBERS)
                assert np.all(ret[nm] == -500) and np.all(sg[nm] == -1) and np.all(ln[nm] == 400) and np.all(np.isnan(xy[nm]))
            if header[0] != 0:                                                             # disable 1: frozen from the first collision on
                frozen = 0
                for m in TRACED:
                    t = eng.maze_debug_trace(m, 400)
                    if not np.all(np.isfinite(t)):
                        continue
                    pos, speed = t[:, 11:13], t[:, 14]
                    stuck = np.flatnonzero(np.all(pos[1:] == pos[:-1], axis=1) & (speed[1:] != 0)) + 1   # a step at speed that moved nothing
                    if stuck.size:
                        assert np.all(pos[stuck[0]:] == pos[stuck[0]]) and np.all(speed[-50:] != 0), (name, m)   # ... and nothing moved after it
                        frozen += 1
                assert frozen >= 1 and xy[1, 0] > header[2], name                             # (the straight-ahead member is one of them)
    assert eng.check_redzones() == 0


# ---- lane placement: one wall out of 64 is the hit, in the first lane, the last lane, the second round of the deal, the last wall -------------------
ZERO_WALL = (150.0, 100.0, 150.0, 100.0)
AT_8 = (68.0, 60.0, 68.0, 140.0)                 # synthetic_maze starts at (60, 100): distance exactly 8.0
AT_7_99 = (67.99, 60.0, 67.99, 140.0)


@pytest.mark.parametrize("slot", (0, 15, 16, 63))
def test_one_hit_among_64_walls_reaches_all_16_lanes(eng, slot):
    from dne_hip import _lib
    header, base_lines = M.synthetic_maze(64)
    th = thetas()
    still, straight, spin = 0, 1, 2
    free = _lib.maze_rollout_host(th, header, base_lines, 400)
    assert not np.array_equal(free[2][straight], header[2:4])                              # without the special wall the navigator gets away
    for wall in (ZERO_WALL, AT_8, AT_7_99):
        lines = base_lines.copy()
        lines[slot] = wall
        hret, hln, hxy, htrace = _lib.maze_rollout_host(th, header, lines, 400, want_trace=True)
        eng.maze_set_walls(header, lines)
        ret, sg, ln = eng.eval_members(NMEM, 400, np.zeros(NMEM, np.uint32))
        xy = eng.maze_final_state(NMEM)
        assert M.same_nan(ret, hret) and M.same_nan(xy, hxy) and np.array_equal(ln, hln), (slot, wall)
        for m in (still, straight, 19):
            assert M.same_nan(eng.maze_debug_trace(m, 400), htrace[m]), (slot, wall, m)
        # what the wall is there for, on the device's results: only this one wall can say so, whichever lane holds it
        finite = [i for i in range(NMEM) if i not in NAN_MEMBERS and i != HUGE]
        if wall is ZERO_WALL:
            assert np.all(xy == header[2:4])                                               # every step of every member collides
        else:
            assert np.all(xy[[still, straight, spin]] == header[2:4])                      # straight ahead: the first step towards it collides, and every later one
        assert np.all(np.isfinite(ret[finite]))
    assert eng.check_redzones() == 0


# ---- one ES step whose returns tie at -500 ---------------------------------------------------------------------------------------------------
def test_one_es_step_with_tied_returns_of_minus_500(oracle):
    from dne_hip import _lib
    header, lines = M.edge_maze("dist_8")
    # theta_0 with a NaN in the noise table under three of the seven pairs: both members of such a pair act NaN and return -500
    tab = noise().copy()
    idx = np.random.RandomState(12).randint(0, 150_000, size=7).astype(np.int64)
    idx = np.sort(idx)
    assert np.all(np.diff(idx) > M.P)                                                      # (the pairs' slices do not overlap)
    for k in (1, 3, 4):
        tab[idx[k] + M.B3] = NAN                                                           # the slice's output-bias entry
    th0 = M.theta0(noise())
    e = _lib.Engine(_lib.KIND_MAZE, 2, max_members=14, record_bc=True, bc_max_steps=400)
    try:
        e.noise_upload(tab)
        e.maze_set_walls(header, lines)
        e.set_theta(th0)
        e.optimizer_reset()
        ret, sg, ln, bc = e.es_eval(idx, 0.02, 400, np.zeros(14, np.uint32), want_bc=True)
        th = np.stack([M.perturbed(th0, tab, int(i), s) for i in idx for s in (0.02, -0.02)])
        hret, hln, hxy, htrace = _lib.maze_rollout_host(th, header, lines, 400, want_trace=True)
        assert M.same_nan(ret.reshape(-1), hret) and np.array_equal(ln.reshape(-1), hln)
        assert np.all(ret[[1, 3, 4]] == -500) and np.all(sg[[1, 3, 4]] == -1) and np.all(ret[[0, 2, 5, 6]] > -500) and np.all(ln == 400)
        # bc through dne_es_eval: the pairs' (x, y) after every step
        assert bc.shape == (14, 400, 2) and M.same_nan(bc, np.ascontiguousarray(htrace[:, :, 11:13]))
        assert M.same_nan(e.maze_final_state(14), hxy)
        # the update: six returns tie at -500 and go through the centered ranks; the NaN table entries are multiplied by the pairs' weight
        # difference, which is exactly 0 only if both members of a pair get one rank -- the oracle's ranks decide, and the device must agree
        e.es_update(idx, ret, sg, "centered_rank", "adam", 0.005, 0.01)
        opt = oracle.Adam(th0, 0.01)
        _, want = opt.update(oracle.es_gradient(tab, idx, hret.reshape(7, 2), M.P), 0.005)
        m, v, t = e.optimizer_get_state()
        assert M.same_nan(e.get_theta(), want) and M.same_nan(m, opt.m) and M.same_nan(v, opt.v) and t == 1
        assert np.flatnonzero(np.isnan(want)).tolist() == [M.B3] and not M.same_nan(want, th0)        # NaN reaches the one parameter it sits under
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- recording capacities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", (5, 0))
def test_bc_capacity_below_the_episode(cap):
    from dne_hip import _lib
    header, lines = M.edge_maze("disable")
    htrace = host("disable", 400)[3]
    e = _lib.Engine(_lib.KIND_MAZE, 2, max_members=NMEM, record_bc=True, bc_max_steps=cap)
    try:
        e.noise_upload(noise())
        upload(e, thetas())
        e.maze_set_walls(header, lines)
        ret, sg, ln, bc = e.eval_members(NMEM, 400, np.zeros(NMEM, np.uint32), want_bc=True)
        rows = max(cap, 1)
        assert bc.shape == (NMEM, rows, 2) and M.same_nan(bc, np.ascontiguousarray(htrace[:, :rows, 11:13]))   # only the first steps are kept
        assert M.same_nan(ret, host("disable", 400)[0]) and np.all(ln == 400)
        assert e.check_redzones() == 0                                                    # nothing was written past the shorter rows
    finally:
        e.close()


def test_all_of_max_members_7_and_walls_set_twice():
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_MAZE, 2, max_members=7, record_bc=True, bc_max_steps=400)
    try:
        e.noise_upload(noise())
        th = thetas()[[1, 3, 5, 13, 14, 19, 22]]
        upload(e, th)
        # 64 walls, then 1 wall: the evaluation reads the one wall, none of the 63 left behind in the buffer
        h64, l64 = M.synthetic_maze(64)
        h1, l1 = M.synthetic_maze(1)
        e.maze_set_walls(h64, l64)
        r64 = e.eval_members(7, 400, np.zeros(7, np.uint32))[0]
        assert M.same_nan(r64, _lib.maze_rollout_host(th, h64, l64, 400)[0])
        e.maze_set_walls(h1, l1)
        hret, hln, hxy, htrace = _lib.maze_rollout_host(th, h1, l1, 400, want_trace=True)
        ret, sg, ln, bc = e.eval_members(7, 400, np.zeros(7, np.uint32), want_bc=True)           # n == max_members, a last wave of three
        assert M.same_nan(ret, hret) and M.same_nan(e.maze_final_state(7), hxy) and np.array_equal(ln, hln)
        assert M.same_nan(bc, np.ascontiguousarray(htrace[:, :, 11:13])) and not M.same_nan(ret, r64)
        for m in (0, 6):
            assert M.same_nan(e.maze_debug_trace(m, 400), htrace[m])
        with pytest.raises(_lib.DneError, match="max_members"):
            e.eval_members(8, 400, np.zeros(8, np.uint32))
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- the math probe on the device -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", (M.MATH_SINCOS_D, M.MATH_ATAN_D, M.MATH_SINCOS_F, M.MATH_ANGLE_F))
def test_device_math_equals_host_math_bit_for_bit(eng, fn):
    from dne_hip import _lib
    x = np.concatenate([M.math_inputs(fn), [np.nan, np.inf, -np.inf]])
    want = _lib.maze_math_host(fn, x)
    got = eng.maze_debug_math(fn, x)
    assert M.same_nan(got, want), int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)))
    assert np.isnan(got[-3, 0]) and np.count_nonzero(np.isnan(got)) <= 6            # NaN from NaN; nothing in the fixed set gives one
    for bad in (-1, 4):
        with pytest.raises(_lib.DneError, match="fn 0..3"):
            eng.maze_debug_math(bad, x[:4])
