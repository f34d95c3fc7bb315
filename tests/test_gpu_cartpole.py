"""GPU: k_cartpole_rollout (csrc/cartpole.h: whole gym.CartPole-v1 episodes in one launch, 16 lanes per member, four members per wave, one wave per
workgroup) on a DNE_KIND_CARTPOLE engine against dne_cartpole_rollout_host -- the same header compiled for the CPU -- BIT FOR BIT: returns,
sign-returns, lengths, final states as doubles, the per-step trace.  Member counts 1, 3, 4, 5, 9 (one row, a workgroup's four members minus one,
exactly four, plus one, a partial third wave), sigma 0, 0.02 and 1.0 over theta_0 from a 200 000-entry table, timestep limits 1, 7, 500, 5000;
one launch whose neighbouring rows end 490 steps apart; five pairs through dne_es_eval, every episode under its own seed; the trace from the
threshold states; the kind's refusals; and the es_gpu.py driver on this engine against the driver on the host-function engine."""
import functools

import numpy as np
import pytest

import cartpole_support as S

pytestmark = pytest.mark.gpu
COUNTS = (1, 3, 4, 5, 9)
LIMITS = (1, 7, 500, 5000)
NMEM = 9


@functools.lru_cache(maxsize=None)
def noise():
    return S.maze_noise()


@functools.lru_cache(maxsize=None)
def bases():
    """base slots: 0 = theta_0, 1 = theta 0 (equal logits: action 0 every step), 2 = the balancing theta"""
    return [S.theta0(noise(), 1234), np.zeros(S.P, np.float32), S.balancing_theta()]


@functools.lru_cache(maxsize=None)
def members():
    """(slot, offset, scale, seed) of the 9 members: theta_0 at sigma 0, +-0.02 and +-1.0, a balancing member among them in every count above 3"""
    rs = np.random.RandomState(5)
    off = rs.randint(0, noise().size - S.P + 1, size=NMEM).astype(np.int64)
    scale = np.array([0.02, -0.02, 0.0, 0.0, 1.0, -1.0, 0.0, 0.02, 1.0], np.float32)
    slot = np.array([0, 0, 0, 2, 0, 0, 1, 0, 0], np.int32)
    off[1] = off[0]                                     # members (0, 1) are an antithetic pair
    off[-1] = noise().size - S.P                        # the last legal slice of the table
    seeds = np.array([0, 1, 2 ** 31, 2 ** 32 - 1, 17, 123456789, 99, 4000000000, 5], np.uint32)
    return slot, off, scale, seeds


@functools.lru_cache(maxsize=None)
def member_thetas():
    slot, off, scale, _ = members()
    return np.stack([S.perturbed(bases()[slot[i]], noise(), int(off[i]), scale[i]) for i in range(NMEM)])


@functools.lru_cache(maxsize=None)
def host(tslimit):
    """the CPU side of the comparison, once per limit: returns, lengths, final states, trace of all 9 members"""
    from dne_hip import _lib
    return _lib.cartpole_rollout_host(member_thetas(), members()[3], tslimit, want_trace=True)


@pytest.fixture(scope="module")
def eng():
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_CARTPOLE, 2, max_members=16)
    e.noise_upload(noise())
    for s, th in enumerate(bases()):
        e.set_theta(th, slot=s)
    yield e
    e.close()


def same32(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def same64(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(S.bits64(a), S.bits64(b))


def test_member_set_is_what_the_docstring_says():
    """held on the host function alone: the episodes differ in length, the balancing member runs all 500 steps, power-0 members are theta_0"""
    ret, ln, state, _ = host(500)
    assert ln[3] == 500 and np.all(ln[[0, 1, 2, 4, 5, 6, 7, 8]] < 500) and len(np.unique(ln)) >= 4 and np.all(ln >= 8)
    assert np.array_equal(ret, ln.astype(np.float32))
    assert np.all((np.abs(state[ln < 500, 0]) > S.X_TH) | (np.abs(state[ln < 500, 2]) > S.TH))             # those episodes ended past a threshold


def test_kernel_equals_host_bit_for_bit(eng):
    slot, off, scale, seeds = members()
    for n in COUNTS:
        eng.set_members(slot[:n], off[:n], scale[:n])
        for tslimit in LIMITS:
            hret, hln, hstate, htrace = host(tslimit)
            ret, sg, ln = eng.eval_members(n, tslimit, seeds[:n])
            print("n", n, "tslimit", tslimit, "lengths", ln.tolist(), "host", hln[:n].tolist())
            assert same32(ret, hret[:n]) and np.array_equal(ln, hln[:n]) and same32(sg, hret[:n]), (n, tslimit)
            assert same64(eng.cartpole_final_state(n), hstate[:n]), (n, tslimit)
            assert np.all(ln <= min(tslimit, 500)) and (tslimit > 7 or np.all(ln == tslimit))
            if n in (5, 9) or tslimit == 7:
                for m in {0, n - 1, min(3, n - 1)}:
                    tr = eng.cartpole_debug_trace(m, tslimit)
                    assert tr.shape == (hln[m], 8) and same64(tr, htrace[m, :hln[m]]), (n, tslimit, m)
                assert same64(eng.cartpole_final_state(n), hstate[:n])      # the trace launches left the evaluation's results alone
        assert eng.check_redzones() == 0
    with pytest.raises(Exception, match="last evaluation ran 9"):
        eng.cartpole_final_state(10)


def test_one_launch_whose_neighbours_differ(eng):
    """two waves of rows that alternate between theta 0 (about 9 steps) and the balancing theta (500 steps), either way round: the rows that
    leave the loop early and the rows that stay do not disturb each other"""
    from dne_hip import _lib
    seeds = (np.arange(8, dtype=np.uint32) * 2654435761 + 12345).astype(np.uint32)
    for first in (1, 2):
        slot = np.array([first if i % 2 == 0 else 3 - first for i in range(8)], np.int32)
        zero = np.zeros(8, np.int64)
        th = np.stack([bases()[s] for s in slot])
        hret, hln, hstate, htrace = _lib.cartpole_rollout_host(th, seeds, 500, want_trace=True)
        short, long_ = slot == 1, slot == 2
        assert np.all(hln[short] < 20) and np.all(hln[long_] == 500)
        eng.set_members(slot, zero, np.zeros(8, np.float32))
        ret, sg, ln = eng.eval_members(8, 500, seeds)
        assert same32(ret, hret) and same32(sg, hret) and np.array_equal(ln, hln) and same64(eng.cartpole_final_state(8), hstate)
        # each member alone gives what it gave among its neighbours
        for m in (0, 1, 5):
            eng.set_members(slot[m:m + 1], zero[:1], np.zeros(1, np.float32))
            r1, _, l1 = eng.eval_members(1, 500, seeds[m:m + 1])
            assert l1[0] == hln[m] and same64(eng.cartpole_final_state(1)[0], hstate[m])
    assert eng.check_redzones() == 0


@pytest.mark.parametrize("sigma", (0.02, 1.0))
def test_pairs_through_es_eval(eng, sigma):
    from dne_hip import _lib
    eng.set_theta(bases()[0])
    idx = np.random.RandomState(9).randint(0, noise().size - S.P + 1, size=5).astype(np.int64)
    seeds = np.random.RandomState(10).randint(0, 2 ** 32, size=10, dtype=np.uint64).astype(np.uint32)
    th = np.stack([S.perturbed(bases()[0], noise(), int(i), s) for i in idx for s in (sigma, -sigma)])
    for tslimit in (500, 7):
        hret, hln, hstate = _lib.cartpole_rollout_host(th, seeds, tslimit)
        ret, sg, ln = eng.es_eval(idx, sigma, tslimit, seeds)
        assert ret.shape == (5, 2) and same32(ret.reshape(-1), hret) and np.array_equal(ln.reshape(-1), hln) and same32(sg.reshape(-1), hret)
        assert same64(eng.cartpole_final_state(10), hstate)
    # the seeds matter: the same pairs under other seeds end elsewhere, as the host says
    other = seeds[::-1].copy()
    eng.es_eval(idx, sigma, 7, other)
    got = eng.cartpole_final_state(10)
    assert same64(got, _lib.cartpole_rollout_host(th, other, 7)[2]) and not same64(got, hstate)
    rec = eng.records_pack(5)                                        # the wire records of the last evaluation
    assert np.array_equal(rec["noise_idx"], idx) and np.all(rec["len"] == 7) and np.all(rec["ret"] == 7.0) and np.all(rec["aux"] == 7.0)
    assert eng.check_redzones() == 0


def test_debug_trace(eng):
    from dne_hip import _lib
    slot = np.array([1, 2], np.int32)
    eng.set_members(slot, np.zeros(2, np.int64), np.zeros(2, np.float32))
    th = np.stack([bases()[1], bases()[2]])
    init = np.array([[0.0, 0.0, 0.0, 0.0], list(S.BALANCE_INIT)])
    hret, hln, hstate, htrace = _lib.cartpole_rollout_host(th, [0, 0], 500, init=init, want_trace=True)
    assert hln.tolist() == [9, 500] and hstate[1, 0] == S.BALANCE_FINAL_X
    for m in (0, 1):                                                 # one short and one 500-step member: every step's observation and state
        tr = eng.cartpole_debug_trace(m, 500, init=init[m])
        assert tr.shape == (hln[m], 8) and same64(tr, htrace[m, :hln[m]])
        assert np.array_equal(tr[:, :4], tr[:, 4:].astype(np.float32).astype(np.float64))
        tr7 = eng.cartpole_debug_trace(m, 7, init=init[m])
        assert tr7.shape == (7, 8) and same64(tr7, htrace[m, :7])
    for st, done in S.threshold_states():                            # ON a threshold goes on, the next double beyond ends at step 1
        for m in (0, 1):
            want = _lib.cartpole_rollout_host(th[m][None], [0], 500, init=np.array([st]))[1][0]
            steps = eng.cartpole_debug_trace(m, 500, init=st).shape[0]
            assert steps == want and (steps == 1) == done, (st, m)
    # init=None: the reset of the seed the member had in the last evaluation
    seeds = np.array([77, 2 ** 32 - 2], np.uint32)
    ret, sg, ln = eng.eval_members(2, 500, seeds)
    hret, hln, hstate, htrace = _lib.cartpole_rollout_host(th, seeds, 500, want_trace=True)
    for m in (0, 1):
        assert ln[m] == hln[m] and same64(eng.cartpole_debug_trace(m, 500), htrace[m, :hln[m]])
    assert eng.check_redzones() == 0


def test_one_es_update_equals_the_update_from_the_host_returns(eng, oracle):
    from dne_hip import _lib
    th0 = bases()[0]
    eng.set_theta(th0)
    eng.optimizer_reset()
    idx = np.random.RandomState(11).randint(0, noise().size - S.P + 1, size=8).astype(np.int64)
    seeds = np.arange(16, dtype=np.uint32) * 977
    ret, sg, ln = eng.es_eval(idx, 0.02, 500, seeds)
    th = np.stack([S.perturbed(th0, noise(), int(i), s) for i in idx for s in (0.02, -0.02)])
    hret = _lib.cartpole_rollout_host(th, seeds, 500)[0].reshape(8, 2)
    assert same32(ret, hret)
    eng.es_update(idx, ret, sg, "centered_rank", "adam", 0.005, 0.01)
    opt = oracle.Adam(th0, 0.01)
    _, want = opt.update(oracle.es_gradient(noise(), idx, hret, S.P), 0.005)
    m, v, t = eng.optimizer_get_state()
    assert same32(eng.get_theta(), want) and same32(m, opt.m) and same32(v, opt.v) and t == 1 and not same32(want, th0)
    eng.set_theta(th0); eng.optimizer_reset()
    assert eng.check_redzones() == 0


def test_refusals(eng):
    from dne_hip import _lib
    with pytest.raises(_lib.DneError, match=r"DNE_KIND_CARTPOLE has 2 actions.*n_actions 18"):
        _lib.Engine(_lib.KIND_CARTPOLE, 18, max_members=4)
    with pytest.raises(_lib.DneError, match=r"bc_final_only is not available on a DNE_KIND_CARTPOLE engine \(kind 5\).*dne_cartpole_final_state"):
        _lib.Engine(_lib.KIND_CARTPOLE, 2, max_members=4, bc_final_only=True)
    fresh = _lib.Engine(_lib.KIND_CARTPOLE, 2, max_members=4)
    try:
        with pytest.raises(_lib.DneError, match="last evaluation"):
            fresh.cartpole_final_state(1)
        fresh.noise_upload(noise())
        with pytest.raises(_lib.DneError, match="max_members"):
            fresh.es_eval(np.zeros(3, np.int64), 0.02, 500, np.zeros(6, np.uint32))
        with pytest.raises(_lib.DneError, match="outside the table"):
            fresh.es_eval(np.array([noise().size - S.P + 1], np.int64), 0.02, 500, np.zeros(2, np.uint32))
        with pytest.raises(_lib.DneError, match="dne_set_members set 0"):
            fresh.eval_members(1, 500, np.zeros(1, np.uint32))
        with pytest.raises(_lib.DneError, match="dne_cartpole_debug_trace: member 0"):
            fresh.cartpole_debug_trace(0)
        assert fresh.check_redzones() == 0
    finally:
        fresh.close()
    slot, off, scale, seeds = members()
    eng.set_members(slot[:4], off[:4], scale[:4])
    one = np.zeros(1, np.uint32)
    with pytest.raises(_lib.DneError, match=r"dne_eval_members: behaviour characterisations are not available on a DNE_KIND_CARTPOLE engine \(kind 5\): bc must be NULL"):
        eng.eval_members(1, 500, one, want_bc=True)
    with pytest.raises(_lib.DneError, match=r"dne_es_eval: behaviour characterisations are not available on a DNE_KIND_CARTPOLE engine"):
        eng.es_eval(np.zeros(1, np.int64), 0.02, 500, np.zeros(2, np.uint32), want_bc=True)
    eng.set_members(slot[:4], off[:4], scale[:4])
    with pytest.raises(_lib.DneError, match="timestep limit"):
        eng.eval_members(1, 0, one)
    calls = {
        "dne_ga_eval": lambda: eng.ga_eval([[1, 2]], 0.01, 10, one),
        "dne_ga_eval_powers": lambda: eng.ga_eval_powers([((1,), (2, 0.1))], 10, one),
        "dne_ga_rebuild": lambda: eng.ga_rebuild(0, [1, 2], 0.01),
        "dne_ga_rebuild_powers": lambda: eng.ga_rebuild_powers(0, ((1,), (2, 0.1))),
        "dne_ga_set_init_scale": lambda: eng.ga_set_init_scale(np.zeros(S.P, np.float32)),
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
        with pytest.raises(_lib.DneError, match=name + r" is not available on a DNE_KIND_CARTPOLE engine \(kind 5\)"):
            call()
    maze_calls = {
        "dne_maze_set_walls": lambda: eng.maze_set_walls(np.zeros(8, np.float32), np.zeros((1, 4), np.float32)),
        "dne_maze_final_state": lambda: eng.maze_final_state(1),
        "dne_maze_debug_trace": lambda: eng.maze_debug_trace(0),
        "dne_maze_debug_math": lambda: eng.maze_debug_math(0, [0.5]),
        "dne_maze_archive_clear": lambda: eng.maze_archive_clear(),
        "dne_maze_novelty": lambda: eng.maze_novelty(1, xy=np.zeros((1, 2), np.float32)),
        "dne_maze_ga_set_init_scale": lambda: eng.maze_ga_set_init_scale(np.zeros(498, np.float32)),
    }
    for name, call in maze_calls.items():
        with pytest.raises(_lib.DneError, match=name + r" needs a DNE_KIND_MAZE engine \(this one: kind 5\)"):
            call()
    # and the cart-pole calls on engines of other kinds
    for kind, nact in ((_lib.KIND_GA, 18), (_lib.KIND_MAZE, 2)):
        other = _lib.Engine(kind, nact, max_members=4)
        try:
            with pytest.raises(_lib.DneError, match=r"dne_cartpole_final_state needs a DNE_KIND_CARTPOLE engine \(this one: kind %d\)" % kind):
                other.cartpole_final_state(1)
            with pytest.raises(_lib.DneError, match="dne_cartpole_debug_trace needs a DNE_KIND_CARTPOLE engine"):
                other.cartpole_debug_trace(0)
        finally:
            other.close()
    # the engine is as usable as before
    hret, hln, hstate, _ = host(500)
    eng.set_members(slot[:4], off[:4], scale[:4])
    ret, sg, ln = eng.eval_members(4, 500, seeds[:4])
    assert same32(ret, hret[:4]) and np.array_equal(ln, hln[:4]) and same64(eng.cartpole_final_state(4), hstate[:4])
    assert eng.check_redzones() == 0


def test_driver_on_the_hip_engine_equals_the_host_function_engine(oracle, tmp_path):
    from dne_hip import _lib, es, es_gpu
    exp = {"game": S.GAME, "model": "SimpleClassifier", "num_test_episodes": 4, "population_size": 16, "timesteps": 10 ** 9,
           "episode_cutoff_mode": 5000, "return_proc_mode": "centered_rank", "l2coeff": 0.005, "mutation_power": 0.02,
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}}

    def table():
        t = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
        t.noise, t._engines = noise(), []
        return t

    hip = _lib.Engine(_lib.KIND_CARTPOLE, 2, max_members=16)
    try:
        a = es_gpu.main(str(tmp_path / "hip"), engine=hip, noise=table(), seed=3, max_iters=2, **exp)
        assert hip.check_redzones() == 0
    finally:
        hip.close()
    b = es_gpu.main(str(tmp_path / "host"), engine=S.CartPoleHostEngine(max_members=16), noise=table(), seed=3, max_iters=2, **exp)
    assert a.it == b.it == 2 and a.timesteps_so_far == b.timesteps_so_far > 0 and a.num_frames == b.num_frames and a.game == S.GAME
    assert same32(a.theta, b.theta) and same32(a.optimizer[0], b.optimizer[0]) and same32(a.optimizer[1], b.optimizer[1]) and a.optimizer[2] == 2
    # the engine the driver builds for itself when none is passed in
    c = es_gpu.main(str(tmp_path / "own"), noise=table(), seed=3, max_iters=2, **exp)
    assert same32(c.theta, b.theta)
