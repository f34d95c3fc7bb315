"""GPU: k_pendulum_rollout<H, TANH> (csrc/pendulum.h: whole pendulum episodes of MujocoPolicy in one launch, one workgroup of H threads per member,
the member's l1/w column in registers, activations through LDS) on a DNE_KIND_PENDULUM engine against dne_pendulum_rollout_host -- the same
header compiled for the CPU -- BIT FOR BIT: returns, sign-returns, lengths, final states and observation statistics as doubles, the per-step
trace.  All six instantiations (H = 64 / 128 / 256 = one, two and four waves, the last with half of the column in accumulator registers; tanh
and relu), the continuous action and 2, 5 and 16 uniform bins; members at sigma 0, +-0.02 and 1.0 over a normc theta from a 200 000-entry
table, the last legal slice of the table among them; action noise on some members (one reading the table's last 200 values) and statistics on
some; timestep limits 1, 7, 200 and 5000; 300 members in one launch (more workgroups than the card runs at once); pairs through dne_es_eval;
tanh_f, norm_angle and the normalisation value by value on the device; one ES update; the kind's refusals; and es.run_master / run_worker
with configurations/humanoid.json's shape on this engine against the same drivers on the host-function engine."""
import functools

import numpy as np
import pytest

import pendulum_support as S

pytestmark = pytest.mark.gpu
SHAPES = ((64, "continuous:", "tanh"), (64, "uniform:5", "relu"), (128, "uniform:16", "tanh"), (128, "continuous:", "relu"),
          (256, "continuous:", "tanh"), (256, "uniform:2", "relu"))
MEAN, STD = np.array([0.1, -0.2, 0.3], np.float32), np.array([0.7, 0.6, 3.0], np.float32)
NMEM = 6
AC_STD = 0.05


@functools.lru_cache(maxsize=None)
def noise():
    return S.maze_noise()


@functools.lru_cache(maxsize=None)
def shape(H, ac_bins, nonlin):
    from dne_hip import _lib, policies
    H, O, mode, nl = policies.mujoco_shape(ac_bins, nonlin, [H, H], "ff")
    return H, O, mode, nl, _lib.pendulum_num_params(H, O)


@functools.lru_cache(maxsize=None)
def bases(H, O):
    """base slots: 0 = a normc theta scaled up so that actions leave +-2 now and then, 1 = theta 0"""
    from dne_hip import policies
    th = policies.normc_flat(H, O, 3)
    th[S.offsets(H, O)[4]:] *= np.float32(150.0)           # out/w: normc(0.01) gives actions of a few hundredths
    return [th, np.zeros_like(th)]


@functools.lru_cache(maxsize=None)
def members(P):
    """(slot, offset, scale, seed, ac_off, flag) of the 6 members"""
    rs = np.random.RandomState(5)
    off = rs.randint(0, noise().size - P + 1, size=NMEM).astype(np.int64)
    scale = np.array([0.02, -0.02, 0.0, 1.0, 0.0, -1.0], np.float32)
    slot = np.array([0, 0, 0, 0, 1, 0], np.int32)
    off[1] = off[0]                                          # members (0, 1) are an antithetic pair
    off[-1] = noise().size - P                               # the last legal slice of the table
    seeds = np.array([0, 1, 2 ** 31, 2 ** 32 - 1, 17, 4000000000], np.uint32)
    ac_off = np.array([0, -1, 1234, noise().size - S.STEPS, -1, 77], np.int64)   # member 3 reads the table's last 200 values
    flag = np.array([1, 0, 0, 1, 1, 0], np.uint8)
    return slot, off, scale, seeds, ac_off, flag


@functools.lru_cache(maxsize=None)
def host(sh, tslimit, options):
    """the CPU side of the comparison, once per shape, limit and (with / without options)"""
    from dne_hip import _lib
    H, O, mode, nl, P = shape(*sh)
    slot, off, scale, seeds, ac_off, flag = members(P)
    th = np.stack([S.perturbed(bases(H, O)[slot[i]], noise(), int(off[i]), scale[i]) for i in range(NMEM)])
    kw = dict(ac_noise_std=AC_STD, table=noise(), ac_off=ac_off, stat_flag=flag) if options else {}
    return _lib.pendulum_rollout_host(th, seeds, H, MEAN, STD, n_out=O, ac_mode=mode, nonlin=nl, tslimit=tslimit, want_trace=True, **kw)


_engines = []


@functools.lru_cache(maxsize=None)
def engine(sh):
    """one engine per shape, made at its first use and closed with the module"""
    from dne_hip import _lib
    H, O, mode, nl, P = shape(*sh)
    e = _lib.Engine(_lib.KIND_PENDULUM, O, max_members=320 if H == 64 else 16, hidden=H, ac_mode=mode, nonlin=nl)
    assert e.P == P
    e.noise_upload(noise())
    for s, th in enumerate(bases(H, O)):
        e.set_theta(th, slot=s)
    e.pendulum_set_ob_stat(MEAN, STD)
    _engines.append(e)
    return e


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    yield
    while _engines:
        _engines.pop().close()
    engine.cache_clear()


def same32(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def same64(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(S.bits(np.asarray(a, np.float64)), S.bits(np.asarray(b, np.float64)))


def test_member_set_is_what_the_docstring_says():
    """held on the host function alone: the clip engages, the bins differ, the noise moves the action, statistics only where flagged"""
    for sh in SHAPES:
        r = host(sh, 200, True)
        tr = r["trace"]
        assert (r["lengths"] == 200).all() and len(np.unique(r["returns"])) >= 5
        assert (np.abs(tr[:4, :, 4]) > 2).any(), sh               # an applied action beyond the torque limit
        assert np.array_equal(r["ob_count"], 200 * members(shape(*sh)[4])[5])
        assert not tr[4, :, 3].any() or shape(*sh)[2] == "uniform"      # theta 0: the continuous action is 0 (bin 0, -2, under uniform bins)
        if shape(*sh)[2] == "uniform":
            assert len(np.unique(tr[:4, :, 3])) >= 2


@pytest.mark.parametrize("sh", SHAPES, ids=lambda s: "%d-%s-%s" % s)
def test_kernel_equals_host_bit_for_bit(sh):
    e = engine(sh)
    slot, off, scale, seeds, ac_off, flag = members(e.P)
    for limit in (1, 7, 200, 5000):
        for options in (True, False):
            want = host(sh, limit, options)
            e.set_members(slot, off, scale)
            if options:
                e.pendulum_set_rollout_options(NMEM, AC_STD, ac_off, flag)
            ret, sg, ln = e.eval_members(NMEM, limit, seeds)
            s, q, c = e.pendulum_ob_stats(NMEM)
            assert np.array_equal(ln, want["lengths"]) and (ln == min(limit, 200)).all(), (limit, options)
            assert same32(ret, want["returns"]) and same32(sg, want["signreturns"]), (limit, options, ret, want["returns"])
            assert same64(e.pendulum_final_state(NMEM), want["state"]), (limit, options)
            assert same64(s, want["ob_sum"]) and same64(q, want["ob_sumsq"]) and np.array_equal(c, want["ob_count"]), (limit, options)
    # the options were for one evaluation only: the next one runs without noise and statistics
    e.set_members(slot, off, scale)
    e.pendulum_set_rollout_options(NMEM, AC_STD, ac_off, flag)
    e.eval_members(NMEM, 200, seeds)
    ret, _, _ = e.eval_members(NMEM, 200, seeds)
    assert same32(ret, host(sh, 200, False)["returns"]) and not e.pendulum_ob_stats(NMEM)[2].any()
    # fewer members than were set, and the trace of each
    ret, _, _ = e.eval_members(2, 200, seeds[:2])
    assert same32(ret, host(sh, 200, False)["returns"][:2])
    for m in (0, 3, 5):
        assert same64(e.pendulum_debug_trace(m, 200), host(sh, 200, False)["trace"][m]), m
    tr = e.pendulum_debug_trace(0, 9, init=[np.pi / 2, 7.9])
    from dne_hip import _lib
    H, O, mode, nl, P = shape(*sh)
    th = S.perturbed(bases(H, O)[0], noise(), int(off[0]), scale[0])
    want = _lib.pendulum_rollout_host(th[None], seeds[:1], H, MEAN, STD, n_out=O, ac_mode=mode, nonlin=nl, tslimit=9, init=[[np.pi / 2, 7.9]], want_trace=True)
    assert tr.shape == (9, 8) and same64(tr, want["trace"][0])
    assert e.check_redzones() == 0


def test_three_hundred_members_in_one_launch():
    """more workgroups than the card runs at once (256 at H = 256; at H = 64 several share a compute unit): every member under its own seed"""
    from dne_hip import _lib
    sh = SHAPES[0]
    e = engine(sh)
    H, O, mode, nl, P = shape(*sh)
    n = 300
    rs = np.random.RandomState(9)
    off = rs.randint(0, noise().size - P + 1, size=n).astype(np.int64)
    scale = rs.choice(np.array([0.02, -0.02, 0.5], np.float32), size=n)
    seeds = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    flag = (rs.rand(n) < 0.3).astype(np.uint8)
    e.set_members(np.zeros(n, np.int32), off, scale)
    e.pendulum_set_rollout_options(n, 0.0, None, flag)
    ret, sg, ln = e.eval_members(n, 60, seeds)
    th = np.stack([S.perturbed(bases(H, O)[0], noise(), int(off[i]), scale[i]) for i in range(n)])
    want = _lib.pendulum_rollout_host(th, seeds, H, MEAN, STD, tslimit=60, stat_flag=flag)
    s, q, c = e.pendulum_ob_stats(n)
    assert same32(ret, want["returns"]) and same32(sg, want["signreturns"]) and (ln == 60).all()
    assert same64(s, want["ob_sum"]) and same64(q, want["ob_sumsq"]) and np.array_equal(c, 60 * flag.astype(np.int32))
    assert same64(e.pendulum_final_state(n), want["state"]) and e.check_redzones() == 0


@pytest.mark.parametrize("sh", (SHAPES[1], SHAPES[4]), ids=lambda s: "%d-%s-%s" % s)
def test_pairs_through_es_eval(sh):
    from dne_hip import _lib
    e = engine(sh)
    H, O, mode, nl, P = shape(*sh)
    idx = np.sort(np.random.RandomState(21).randint(0, noise().size - P + 1, size=3)).astype(np.int64)
    seeds = np.array([3, 1 << 31, 77, 5, 2 ** 32 - 1, 9], np.uint32)
    ac_off = np.array([5, 6, -1, 100, 200, 300], np.int64)
    flag = np.array([0, 1, 1, 0, 0, 1], np.uint8)
    e.set_theta(bases(H, O)[0])
    e.pendulum_set_rollout_options(6, AC_STD, ac_off, flag)
    ret, sg, ln = e.es_eval(idx, 0.02, 200, seeds)
    th = np.stack([S.perturbed(bases(H, O)[0], noise(), int(i), s) for i in idx for s in (0.02, -0.02)])
    want = _lib.pendulum_rollout_host(th, seeds, H, MEAN, STD, n_out=O, ac_mode=mode, nonlin=nl, ac_noise_std=AC_STD, table=noise(), ac_off=ac_off, stat_flag=flag)
    assert ret.shape == (3, 2) and same32(ret.reshape(-1), want["returns"]) and same32(sg.reshape(-1), want["signreturns"]) and (ln == 200).all()
    s, q, c = e.pendulum_ob_stats(6)
    assert same64(s, want["ob_sum"]) and same64(q, want["ob_sumsq"]) and np.array_equal(c, want["ob_count"])
    assert e.profile()["env_steps"] == 1200 and e.check_redzones() == 0


def test_math_on_the_device_value_by_value():
    from dne_hip import _lib
    e = engine(SHAPES[0])
    xs = np.arange(0, 2 ** 32, 4099 * 16, dtype=np.uint64).astype(np.uint32).view(np.float32)
    seam = []
    for v in (np.float32(2.0 ** -12), np.float32(10.0), np.float32(1.17549435e-38), np.float32(1e-45)):
        seam += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(np.inf))]
    xs = np.concatenate([xs, np.array(seam + [0.0, np.inf], np.float32), -np.array(seam + [0.0, np.inf], np.float32)]).astype(np.float64)
    assert same64(e.pendulum_debug_math("tanh", xs), _lib.pendulum_math_host("tanh", xs))
    th = np.concatenate([np.random.RandomState(2).uniform(-90, 90, 20000), [np.pi, -np.pi, 0.0, 1e30, -1e30, np.inf, np.nan]])
    assert same64(e.pendulum_debug_math("norm", th), _lib.pendulum_math_host("norm", th))
    ob = np.concatenate([np.random.RandomState(4).uniform(-9, 9, 5000), [np.inf, -np.inf, np.nan, 0.3]])
    for a, b in ((0.3, 0.7), (0.3, 0.0), (0.0, np.nan), (np.nan, 1.0), (-1.5, 1e-30)):
        dev, hst = e.pendulum_debug_math("normalise", ob, a, b), _lib.pendulum_math_host("normalise", ob, a, b)
        # (a NaN is a NaN on both sides; which NaN an arithmetic operation gives -- sign, payload -- is the processor's and no part of the contract)
        assert np.array_equal(np.isnan(dev), np.isnan(hst)) and same64(dev[~np.isnan(dev)], hst[~np.isnan(hst)]), (a, b)


def test_one_es_update_equals_the_update_from_the_host_returns(oracle):
    from dne_hip import _lib
    sh = SHAPES[0]
    e = engine(sh)
    H, O, mode, nl, P = shape(*sh)
    th0 = bases(H, O)[0]
    e.set_theta(th0)
    e.optimizer_reset()
    idx = np.random.RandomState(11).randint(0, noise().size - P + 1, size=8).astype(np.int64)
    seeds = np.arange(16, dtype=np.uint32) * 977
    ret, sg, ln = e.es_eval(idx, 0.02, 200, seeds)
    th = np.stack([S.perturbed(th0, noise(), int(i), s) for i in idx for s in (0.02, -0.02)])
    hret = _lib.pendulum_rollout_host(th, seeds, H, MEAN, STD)["returns"].reshape(8, 2)
    assert same32(ret, hret)
    e.es_update(idx, ret, sg, "centered_rank", "adam", 0.005, 0.01)
    opt = oracle.Adam(th0, 0.01)
    _, want = opt.update(oracle.es_gradient(noise(), idx, hret, P), 0.005)
    m, v, t = e.optimizer_get_state()
    assert same32(e.get_theta(), want) and same32(m, opt.m) and same32(v, opt.v) and t == 1 and not same32(want, th0)
    e.set_theta(th0); e.optimizer_reset()
    assert e.check_redzones() == 0


def test_refusals():
    from dne_hip import _lib
    mk = lambda **kw: _lib.Engine(_lib.KIND_PENDULUM, kw.pop("n", 1), max_members=4, **dict(dict(hidden=64, ac_mode=0, nonlin=0), **kw))
    for kw, text in ((dict(hidden=96), r"width 64, 128 or 256; hidden width 96 is refused"), (dict(hidden=0), "hidden width 0"),
                     (dict(ac_mode=2), "mode 2 is refused"), (dict(nonlin=2), "nonlinearity 2 is refused"),
                     (dict(n=2), "n_actions 2 under mode 0"), (dict(n=1, ac_mode=1), "n_actions 1 under mode 1"), (dict(n=17, ac_mode=1), "n_actions 17"),
                     (dict(bc_final_only=True), r"not available on a DNE_KIND_PENDULUM engine \(kind 6\).*dne_pendulum_final_state"),
                     (dict(record_bc=True), r"not available on a DNE_KIND_PENDULUM engine \(kind 6\)")):
        with pytest.raises(_lib.DneError, match=text):
            mk(**kw)
    P = _lib.pendulum_num_params(64, 1)
    fresh = mk()
    try:
        one, idx1, two = np.zeros(1, np.uint32), np.array([5], np.int64), np.zeros(2, np.uint32)
        with pytest.raises(_lib.DneError, match="last evaluation"):
            fresh.pendulum_final_state(1)
        with pytest.raises(_lib.DneError, match="last evaluation"):
            fresh.pendulum_ob_stats(1)
        with pytest.raises(_lib.DneError, match="noise table not uploaded"):
            fresh.pendulum_set_rollout_options(2, 0.01, np.zeros(2, np.int64), None)
        fresh.noise_upload(noise())
        with pytest.raises(_lib.DneError, match="NaN until dne_pendulum_set_ob_stat"):       # policies.py:138-141: the statistics start as NaN
            fresh.es_eval(idx1, 0.02, 200, two)
        fresh.set_members(np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.float32))
        with pytest.raises(_lib.DneError, match="NaN until dne_pendulum_set_ob_stat"):
            fresh.pendulum_debug_trace(0)
        fresh.pendulum_set_ob_stat(MEAN, STD)
        with pytest.raises(_lib.DneError, match="max_members"):
            fresh.es_eval(np.zeros(3, np.int64), 0.02, 200, np.zeros(6, np.uint32))
        with pytest.raises(_lib.DneError, match="outside the table"):
            fresh.es_eval(np.array([noise().size - P + 1], np.int64), 0.02, 200, two)
        with pytest.raises(_lib.DneError, match=r"member 1 reads its 200 action-noise values from offset %d, past the noise table" % (noise().size - 199)):
            fresh.pendulum_set_rollout_options(2, 0.01, np.array([noise().size - 200, noise().size - 199], np.int64), None)
        fresh.pendulum_set_rollout_options(4, 0.01, np.zeros(4, np.int64), None)
        with pytest.raises(_lib.DneError, match="was given 4 members, this evaluation runs 2"):
            fresh.es_eval(idx1, 0.02, 200, two)
        fresh.pendulum_set_rollout_options(2, 0.01, None, None)                               # (clears the pending ones)
        with pytest.raises(_lib.DneError, match=r"dne_es_eval: behaviour characterisations are not available on a DNE_KIND_PENDULUM engine \(kind 6\): bc must be NULL"):
            fresh.es_eval(idx1, 0.02, 200, two, want_bc=True)
        with pytest.raises(_lib.DneError, match="timestep limit"):
            fresh.eval_members(1, 0, one)
        with pytest.raises(_lib.DneError, match="dne_pendulum_debug_trace: member 7"):
            fresh.pendulum_debug_trace(7)
        calls = {
            "dne_ga_eval": lambda: fresh.ga_eval([[1, 2]], 0.01, 10, one),
            "dne_ga_rebuild": lambda: fresh.ga_rebuild(0, [1, 2], 0.01),
            "dne_ref_pass": lambda: fresh.ref_pass(1),
            "dne_env_reset": lambda: fresh.env_reset(one),
            "dne_env_step": lambda: fresh.env_step(np.zeros(1, np.int32)),
            "dne_act": lambda: fresh.act(1),
            "dne_novelty": lambda: fresh.novelty([], np.zeros((1, 128), np.uint8), 1),
        }
        for name, call in calls.items():
            with pytest.raises(_lib.DneError, match=name + r" is not available on a DNE_KIND_PENDULUM engine \(kind 6\)"):
                call()
        with pytest.raises(_lib.DneError, match=r"dne_maze_final_state needs a DNE_KIND_MAZE engine \(this one: kind 6\)"):
            fresh.maze_final_state(1)
        with pytest.raises(_lib.DneError, match=r"dne_cartpole_final_state needs a DNE_KIND_CARTPOLE engine \(this one: kind 6\)"):
            fresh.cartpole_final_state(1)
        # and it is as usable as before
        ret, _, ln = fresh.es_eval(idx1, 0.02, 200, two)
        assert (ln == 200).all() and (ret < 0).all()
        assert fresh.check_redzones() == 0
    finally:
        fresh.close()
    for kind, nact in ((_lib.KIND_GA, 18), (_lib.KIND_CARTPOLE, 2)):
        other = _lib.Engine(kind, nact, max_members=4)
        try:
            for name, call in (("dne_pendulum_set_ob_stat", lambda: other.pendulum_set_ob_stat(MEAN, STD)),
                               ("dne_pendulum_set_rollout_options", lambda: other.pendulum_set_rollout_options(1)),
                               ("dne_pendulum_ob_stats", lambda: other.pendulum_ob_stats(1)),
                               ("dne_pendulum_final_state", lambda: other.pendulum_final_state(1)),
                               ("dne_pendulum_debug_trace", lambda: other.pendulum_debug_trace(0)),
                               ("dne_pendulum_debug_math", lambda: other.pendulum_debug_math("tanh", [0.5]))):
                with pytest.raises(_lib.DneError, match=name + r" needs a DNE_KIND_PENDULUM engine \(this one: kind %d\)" % kind):
                    call()
        finally:
            other.close()


@pytest.mark.parametrize("prob, ac_std", [(0.5, 0.01)])
def test_drivers_on_the_hip_engine_equal_the_host_function_engine(oracle, tmp_path, prob, ac_std):
    """es.run_master + run_worker, humanoid.json's shape at H = 64 and population 8, two iterations with evaluation episodes: every Result,
    every Task (the observation statistics among its fields) and the returned theta equal those of the host-function engines"""
    import es_driver_support as D
    from dne_hip import _lib, es
    tab = es.SharedNoiseTable(count=400_000)
    exp = S.humanoid_exp(pop=8, calc_obstat_prob=prob, ac_noise_std=ac_std, eval_prob=1.0)
    # (a worker seed of this test's own, and only that worker's Results: the wire spy sits on the class, and a worker thread that an earlier
    # test of the session left looping would show up in it)
    wid = np.random.RandomState(1234).randint(2 ** 31)
    mine = lambda run: run._replace(pushed=[(t, r) for t, r in run.pushed if r.worker_id == wid])
    want = mine(D.run_driver(es, exp, S.PendulumHostEngine(), S.PendulumHostEngine(), tab, tmp_path / "host", 2, worker_seed=1234))
    tab = es.SharedNoiseTable(count=400_000)
    mk = lambda: _lib.Engine(_lib.KIND_PENDULUM, 1, max_members=8, hidden=64, ac_mode="continuous", nonlin="tanh")
    me, we = mk(), mk()
    try:
        got = mine(D.run_driver(es, exp, me, we, tab, tmp_path / "hip", 2, worker_seed=1234))
        assert me.check_redzones() == 0 and we.check_redzones() == 0
    finally:
        me.close(); we.close()
    D.assert_same_run(want, got, "pendulum drivers")
    for (_, w), (_, g) in zip(want.pushed, got.pushed):
        assert (w.ob_sum is None) == (g.ob_sum is None)
        if w.ob_sum is not None:
            assert same32(w.ob_sum, g.ob_sum) and same32(w.ob_sumsq, g.ob_sumsq)
    for w, g in zip(want.tasks, got.tasks):
        assert same32(w.ob_mean, g.ob_mean) and same32(w.ob_std, g.ob_std)
    assert any(r.ob_count for _, r in got.pushed if r.eval_length is None)
