"""GPU: the Deep GA with MujocoPolicy (csrc/mujoco_ga.h) on DNE_KIND_PENDULUM and DNE_KIND_MJMAZE engines against the host twins, BIT FOR BIT
(a NaN -- a column whose squares sum to 0 -- at the same places): k_mujoco_ga_colscale + k_mujoco_ga_build / _promote and get_parent at hidden
64 for every output count class, once each at 128 and 256, T = 1, 3, 5, an index that ends exactly at the table's end, a zero column
planted in the table; dne_mujoco_ga_eval (k_mujoco_ga_roots + the kind's rollout kernel over the bank) against the rollout twin on
members_host's thetas -- returns, lengths, final states, observation sums -- with and without action noise and statistics flags; a root
through its scratch slot against set_theta of the host root; three generations against the host engine; ga_mujoco's drivers on the HIP engine
against the same drivers on the host engine; the refusals.  The noise table is 2^18 floats; tslimit 20 except where a whole episode is said."""
import numpy as np
import pytest

import mujoco_ga_support as S

pytestmark = pytest.mark.gpu

P6, P7 = S.KIND_PENDULUM, S.KIND_MJMAZE
# (kind, hidden, outputs, action mode): hidden 64 for every output count class, once each at 128 and 256
CASES = ((P6, 64, 1, "continuous"), (P6, 64, 2, "uniform"), (P6, 64, 16, "uniform"), (P7, 64, 2, "continuous"), (P7, 64, 16, "uniform"),
         (P6, 128, 1, "continuous"), (P7, 256, 2, "continuous"))
IDS = ["%s-%d-%d" % ("pendulum" if c[0] == P6 else "mjmaze", c[1], c[2]) for c in CASES]
ZERO_AT, T_MAX, SIGMA, LIMIT = 777, 5, 0.02, 20


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def pair(request):
    """(case, table, device engine, host engine) on a table with column O - 1 of out/w zeroed in the slice at ZERO_AT; bank reserved for 5"""
    kind, H, O, mode = request.param
    tab = S.zero_column_table(kind, H, O, ZERO_AT, 2, O - 1)
    dev = S.device_engine(kind, H, O, mode, max_members=16, tab=tab)
    host = S.host_engine(kind, H, O, mode, max_members=16, count=0)
    host.noise_upload(tab)
    for e in (dev, host):
        S.set_stat(e, kind)
        e.mujoco_ga_reserve(T_MAX)
    yield request.param, tab, dev, host
    assert dev.check_redzones() == 0
    dev.close()


def bank_of(e):
    T = e.mujoco_ga_parents()
    return np.stack([e.mujoco_ga_get_parent(j) for j in range(T)]) if T else np.zeros((0, e.P), np.float32)


def chains_for(tab, P, T):
    """T chains of 1..4 seeds: the table's end, its start and the slice with the zero column among the indices"""
    rs = np.random.RandomState(3 + T + P)
    seeds = [int(v) for v in rs.randint(0, tab.size - P + 1, size=16)]
    pool = [(tab.size - P, ), (seeds[0], tab.size - P), (ZERO_AT, seeds[1], seeds[2]), (0, seeds[3], seeds[4], seeds[5]), (seeds[6], 0)]
    return pool[:T]


def test_symbols_exist():
    from dne_hip import _lib, ga_mujoco   # noqa: F401
    assert all(hasattr(_lib.load(), "dne_mujoco_ga_" + n) for n in ("reserve", "build", "eval", "promote", "parents", "get_parent"))


# ---- build, promote, get_parent -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 3, 5))
def test_build_and_promote_equal_the_host_twins(pair, T):
    (kind, H, O, mode), tab, dev, host = pair
    from dne_hip import _lib
    P = dev.P
    assert P == S.num_params(kind, H, O)
    genomes = [S.chain_genome(c, SIGMA) for c in chains_for(tab, P, T)]
    for e in (dev, host):
        e.mujoco_ga_build(genomes)
    got = bank_of(dev)
    assert dev.mujoco_ga_parents() == T and S.same(got, bank_of(host))
    for j, g in enumerate(genomes):
        assert S.same(got[j], _lib.mujoco_ga_theta_host(tab, kind, H, O, g))
    assert np.isnan(got).any() == (T >= 3)                                  # the zero column is in the third chain, and only there
    if T >= 3:
        w0, K, C, _ = S.blocks(kind, H, O)[0][2]
        where = np.zeros(P, bool)
        where[w0 + (O - 1) + C * np.arange(K)] = True
        assert np.array_equal(np.isnan(got[2]), where) and not np.isnan(np.delete(got, 2, axis=0)).any()
    # promotion over the double buffer: kept parents that move, one source named twice, children at the table's end, a root, T_new != T
    T_new = 4 if T == 5 else 5
    rs = np.random.RandomState(T)
    parent = np.array([T - 1, 0, 0, -1, (T - 1) // 2][:T_new], np.int32)
    idx = np.array([-1, -3, tab.size - P, tab.size - P, int(rs.randint(0, tab.size - P + 1))][:T_new], np.int64)
    power = np.array([0.0, 5.0, SIGMA, 7.0, -SIGMA][:T_new], np.float32)
    for e in (dev, host):
        e.mujoco_ga_promote(parent, idx, power)
    after = bank_of(dev)
    assert dev.mujoco_ga_parents() == T_new and S.same(after, bank_of(host))
    assert S.same(after, _lib.mujoco_ga_members_host(tab, kind, H, O, got, parent, idx, power))
    assert S.same(after[0], got[T - 1]) and S.same(after[1], got[0]) and S.same(after[2], S.perturbed(got[0], tab, tab.size - P, SIGMA))
    assert S.same(after[3], S.root_np(tab, kind, H, O, tab.size - P))


@pytest.mark.parametrize("kind", (P6, P7))
def test_a_second_reserve_past_max_members_sizes_every_array_again(kind):
    """reserve small and build, then reserve more parents than max_members and build T = T_max: the chain arrays of the first build are sized
    for the first reserve and must not be kept -- every slot equals the host twin, no buffer's red zone is touched; promotion at T_max too"""
    from dne_hip import _lib
    tab, M, T1, T2 = S.table(), 4, 2, 11
    n_out = 1 if kind == P6 else 2
    e = S.device_engine(kind, max_members=M)
    P = e.P
    rs = np.random.RandomState(21)
    chains = [tuple(int(v) for v in rs.randint(0, tab.size - P + 1, size=1 + j % 3)) for j in range(T2)]
    chains[-1] = (tab.size - P, 0)
    e.mujoco_ga_reserve(T1)
    e.mujoco_ga_build([S.chain_genome(c, SIGMA) for c in chains[:T1]])
    assert e.check_redzones() == 0
    e.mujoco_ga_reserve(T2)
    assert e.mujoco_ga_parents() == 0                                        # it starts over with an empty bank
    e.mujoco_ga_build([S.chain_genome(c, SIGMA) for c in chains])
    assert e.check_redzones() == 0 and e.mujoco_ga_parents() == T2
    want = np.stack([_lib.mujoco_ga_theta_host(tab, kind, 64, n_out, S.chain_genome(c, SIGMA)) for c in chains])
    assert S.same(bank_of(e), want)
    parent, idx = np.arange(T2, dtype=np.int32)[::-1].copy(), np.where(np.arange(T2) % 2 == 0, -1, tab.size - P).astype(np.int64)
    e.mujoco_ga_promote(parent, idx, np.full(T2, SIGMA, np.float32))
    assert e.check_redzones() == 0
    assert S.same(bank_of(e), _lib.mujoco_ga_members_host(tab, kind, 64, n_out, want, parent, idx, np.full(T2, SIGMA, np.float32)))
    e.mujoco_ga_reserve(T1)                                                  # and smaller again
    e.mujoco_ga_build([S.chain_genome(c, SIGMA) for c in chains[:T1]])
    assert e.check_redzones() == 0 and S.same(bank_of(e), want[:T1])
    e.close()


# ---- evaluation -----------------------------------------------------------------------------------------------------------------------------------------
def members12(tab, P, T):
    """12 members over a bank of T: roots (the table's end among them) and children mixed"""
    rs = np.random.RandomState(77 + P)
    parent = np.array([-1, 0, T - 1, -1, 1 % T, 0, -1, T - 1, 0, 1 % T, -1, 0], np.int32)
    idx = rs.randint(0, tab.size - P + 1, size=12).astype(np.int64)
    idx[0], idx[2] = tab.size - P, tab.size - P
    power = np.where(np.arange(12) % 3 == 0, np.float32(0.05), np.float32(SIGMA)).astype(np.float32)
    return parent, idx, power


def run_both(pair, parent, idx, power, limit, noisy, flags):
    (kind, H, O, mode), tab, dev, host = pair
    n = len(parent)
    steps, adim = (200, 1) if kind == P6 else (400, 2)
    seeds = (np.arange(n) * 2654435761 % 2 ** 32).astype(np.uint32)
    rs = np.random.RandomState(n + int(noisy))
    off = rs.randint(0, tab.size - steps * adim + 1, size=n).astype(np.int64) if noisy else None
    if noisy:
        off[0] = tab.size - steps * adim
    flag = (np.arange(n) % 2 == 0).astype(np.uint8) if flags else None
    out = []
    for e in (dev, host):
        set_options, ob_stats, final = S.engine_calls(e, kind)
        if noisy or flags:
            set_options(n, 0.1 if noisy else 0.0, off, flag)
        r = e.mujoco_ga_eval(parent, idx, power, limit, seeds)
        out.append((r, ob_stats(n), final(n)))
    (rd, sd, fd), (rh, sh, fh) = out
    for a, b in zip(rd + sd + (fd, ), rh + sh + (fh, )):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return rd, sd, fd


@pytest.mark.parametrize("noisy,flags", ((False, False), (True, True)))
def test_eval_equals_the_rollout_twin_on_the_members_twin(pair, noisy, flags):
    (kind, H, O, mode), tab, dev, host = pair
    genomes = [S.chain_genome(c, SIGMA) for c in chains_for(tab, dev.P, 2)]          # (no zero column: the episodes should differ)
    for e in (dev, host):
        e.mujoco_ga_build(genomes)
    parent, idx, power = members12(tab, dev.P, 2)
    (ret, _, ln), (s, q, c), final = run_both(pair, parent, idx, power, LIMIT, noisy, flags)
    assert len({row.tobytes() for row in final}) > 6 and (ln == LIMIT).all()       # (the maze pays at step 400 only: the final states tell the episodes apart)
    assert (c[::2] == LIMIT).all() and (c[1::2] == 0).all() if flags else (c == 0).all()
    run_both(pair, parent[:1], idx[:1], power[:1], LIMIT, noisy, flags)             # n = 1: a root alone
    run_both(pair, parent[1:2], idx[1:2], power[1:2], 1, False, False)              # n = 1: a child alone, one step
    assert S.same(bank_of(dev), bank_of(host))                                      # an evaluation leaves the bank alone


@pytest.mark.parametrize("kind", (P6, P7))
def test_one_whole_episode_case_a_kind(kind):
    """hidden 64 under the continuous action, four members (two roots, two children), the environment's own limit"""
    case, tab = (kind, 64, 1 if kind == P6 else 2, "continuous"), S.table()
    dev, host = S.device_engine(kind, max_members=4), S.host_engine(kind, max_members=4)
    for e in (dev, host):
        S.set_stat(e, kind)
        e.mujoco_ga_reserve(2)
        e.mujoco_ga_build([S.chain_genome(c, SIGMA) for c in chains_for(tab, dev.P, 2)])
    parent, idx, power = members12(tab, dev.P, 2)
    own = 200 if kind == P6 else 400
    (ret, _, ln), _, _ = run_both((case, tab, dev, host), parent[:4], idx[:4], power[:4], own, True, True)
    assert (ln == own).all() and dev.check_redzones() == 0
    dev.close()


def test_a_root_through_its_scratch_slot_is_set_theta_of_the_host_root(pair):
    (kind, H, O, mode), tab, dev, host = pair
    from dne_hip import _lib
    idx = np.array([tab.size - dev.P, 4242], np.int64)
    seeds = np.array([5, 6], np.uint32)
    ret, sg, ln = dev.mujoco_ga_eval([-1, -1], idx, [0.0, 0.0], LIMIT, seeds)
    _, _, final = S.engine_calls(dev, kind)
    state = final(2)
    for i in range(2):
        dev.set_theta(_lib.mujoco_ga_theta_host(tab, kind, H, O, (int(idx[i]), )), 0)
        dev.set_members(np.zeros(1, np.int32), idx[i:i + 1], np.zeros(1, np.float32))
        r1, s1, l1 = dev.eval_members(1, LIMIT, seeds[i:i + 1])
        assert r1.view(np.uint32)[0] == ret.view(np.uint32)[i] and l1[0] == ln[i] and s1.view(np.uint32)[0] == sg.view(np.uint32)[i]
        assert np.array_equal(final(1)[0].view(np.uint8), state[i].view(np.uint8))


def test_generation_zero_and_two_promoted_generations_equal_the_host_engine(pair):
    (kind, H, O, mode), tab, dev, host = pair
    P, n, T = dev.P, 8, 3
    rs = np.random.RandomState(9)
    seeds = rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    parent = np.full(n, -1, np.int32)
    chains = [()] * n
    bank_chains = []
    for gen in range(3):
        idx = rs.randint(0, tab.size - P + 1, size=n).astype(np.int64)
        if gen == 0:
            idx[3] = tab.size - P
        outs = [e.mujoco_ga_eval(parent, idx, np.full(n, SIGMA, np.float32), LIMIT, seeds) for e in (dev, host)]
        for a, b in zip(*outs):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), gen
        chains = [(bank_chains[p] if p >= 0 else ()) + (int(i), ) for p, i in zip(parent, idx)]
        order = np.argsort(-outs[0][0], kind="stable")[:T]
        # the new parents: the best three children, each from its own parent (generation 0: roots), and the old parent 0 kept at the end
        pp = [int(parent[i]) for i in order] + ([0] if bank_chains else [])
        pi = [int(idx[i]) for i in order] + ([-1] if bank_chains else [])
        new_chains = [chains[i] for i in order] + ([bank_chains[0]] if bank_chains else [])
        for e in (dev, host):
            e.mujoco_ga_promote(pp, pi, np.full(len(pp), SIGMA, np.float32))
        bank_chains = new_chains
        got = bank_of(dev)
        assert S.same(got, bank_of(host))
        assert S.same(got, np.stack([S.genome_np(tab, kind, H, O, S.chain_genome(c, SIGMA)) for c in bank_chains]))
        parent = rs.randint(0, len(bank_chains), size=n).astype(np.int32)
    assert max(len(c) for c in bank_chains) == 3


# ---- the drivers ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", (P6, P7))
def test_the_drivers_on_the_hip_engine_equal_the_drivers_on_the_host_engine(kind, tmp_path):
    from dne_hip import es
    exp = S.ga_exp(kind, pop=8, population_size=4, num_elites=2, calc_obstat_prob=0.5)
    runs = []
    for make in (S.device_engine, S.host_engine):
        noise = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
        noise.noise, noise._engines = S.table(), []
        me, we = make(kind, max_members=8), make(kind, max_members=8)
        log_dir = tmp_path / make.__name__
        log_dir.mkdir()
        runs.append(S.run_ga(exp, me, we, noise, log_dir, 2))
        if make is S.device_engine:
            assert we.mujoco_ga_parents() == 4 and me.check_redzones() == 0 and we.check_redzones() == 0
            me.close(); we.close()
    S.assert_same_ga_runs(runs[1], runs[0], "ga_mujoco on the HIP engine against the host engine")
    assert sum(r.ob_count for _, r in runs[0]["pushed"] if r.eval_length is None) > 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", (P6, P7))
def test_device_refusals_by_their_words(kind):
    from dne_hip import _lib
    tab = S.table()
    e = _lib.Engine(kind, 1 if kind == P6 else 2, max_members=4, hidden=64)
    P = e.P
    seeds = np.zeros(4, np.uint32)

    def refused(f, *a):
        with pytest.raises(_lib.DneError) as ei:
            f(*a)
        return str(ei.value)
    assert refused(e.mujoco_ga_build, [(0, )]) == "dne_mujoco_ga_build: no bank (dne_mujoco_ga_reserve comes first)"
    assert refused(e.mujoco_ga_eval, [-1], [0], [0.0], LIMIT, seeds[:1]) == "dne_mujoco_ga_eval: no bank (dne_mujoco_ga_reserve comes first)"
    assert refused(e.mujoco_ga_promote, [-1], [0], [0.0]) == "dne_mujoco_ga_promote: no bank (dne_mujoco_ga_reserve comes first)"
    assert refused(e.mujoco_ga_get_parent, 0) == "dne_mujoco_ga_get_parent: no bank (dne_mujoco_ga_reserve comes first)"
    assert "T_max = 0 outside" in refused(e.mujoco_ga_reserve, 0)
    e.mujoco_ga_reserve(2)
    assert refused(e.mujoco_ga_build, [(0, )]) == "dne_mujoco_ga_build: noise table not uploaded (dne_noise_upload)"
    e.noise_upload(tab)
    if kind == P7:
        assert refused(e.mujoco_ga_eval, [-1], [0], [0.0], LIMIT, None) == "dne_mujoco_ga_eval: no maze loaded (dne_maze_set_walls comes before an evaluation)"
        e.maze_set_walls(*S.MS.fixture_maze())
    assert refused(e.mujoco_ga_eval, [-1], [0], [0.0], LIMIT, seeds[:1]) == \
        "dne_mujoco_ga_eval: the observation statistics of a %s engine are NaN until dne_%s_set_ob_stat is called" % (
            ("DNE_KIND_PENDULUM", "pendulum") if kind == P6 else ("DNE_KIND_MJMAZE", "mjmaze"))
    S.set_stat(e, kind)
    assert refused(e.mujoco_ga_eval, [0], [0], [0.0], LIMIT, seeds[:1]) == "dne_mujoco_ga_eval: member 0: parent 0 on an empty bank"
    assert refused(e.mujoco_ga_build, [(0, ), (1, ), (2, )]) == "dne_mujoco_ga_build: T = 3 outside [1, T_max = 2]"
    assert refused(e.mujoco_ga_build, [(0, ), ()]) == "dne_mujoco_ga_build: genome 1: empty chain"
    assert refused(e.mujoco_ga_build, [(0, (tab.size - P + 1, 0.1))]) == \
        "dne_mujoco_ga_build: genome 0: noise index %d + P = %d outside the table of %d" % (tab.size - P + 1, P, tab.size)
    e.mujoco_ga_build([(0, ), (5, (9, SIGMA))])
    bank = bank_of(e)
    assert refused(e.mujoco_ga_eval, [1, 2], [0, 0], [0.0, 0.0], LIMIT, seeds[:2]) == "dne_mujoco_ga_eval: member 1: parent 2, the bank holds 2"
    assert refused(e.mujoco_ga_eval, [0], [tab.size - P + 1], [0.0], LIMIT, seeds[:1]) == \
        "dne_mujoco_ga_eval: member 0: noise index %d + P = %d outside the table of %d" % (tab.size - P + 1, P, tab.size)
    assert refused(e.mujoco_ga_eval, [0], [-1], [0.0], LIMIT, seeds[:1]) == \
        "dne_mujoco_ga_eval: member 0: the kept form (parent 0, idx -1) is for promotion only, an evaluation takes power 0 at a real index"
    assert refused(e.mujoco_ga_eval, [0] * 5, [0] * 5, [0.0] * 5, LIMIT, np.zeros(5, np.uint32)) == "dne_mujoco_ga_eval: n = 5 outside [1, max_members = 4]"
    assert refused(e.mujoco_ga_promote, [0, 1, 0], [-1, -1, -1], [0.0] * 3) == "dne_mujoco_ga_promote: T = 3 outside [1, T_max = 2]"
    assert refused(e.mujoco_ga_promote, [2], [-1], [0.0]) == "dne_mujoco_ga_promote: member 0: parent 2, the bank holds 2"
    assert refused(e.mujoco_ga_get_parent, 2) == "dne_mujoco_ga_get_parent: parent 2, the bank holds 2"
    if kind == P6:
        assert refused(e.mujoco_ga_eval, [0], [0], [0.0], LIMIT, None) == \
            "dne_mujoco_ga_eval: a DNE_KIND_PENDULUM engine resets every member from its environment seed, env_seed is NULL"
    assert S.same(bank_of(e), bank) and e.mujoco_ga_parents() == 2                       # every refusal left the bank as it was
    # the Atari genome calls stay refused, word for word
    name = "DNE_KIND_PENDULUM engine (kind 6): the pendulum" if kind == P6 else "DNE_KIND_MJMAZE engine (kind 7): MujocoPolicy on the hard maze"
    for call, f in (("dne_ga_eval", lambda: e.ga_eval([[0]], SIGMA, LIMIT, seeds[:1])), ("dne_ga_rebuild", lambda: e.ga_rebuild(0, [0], SIGMA))):
        assert refused(f) == "%s is not available on a %s has no Atari frames, reference batch, genomes or byte BCs" % (call, name)
    assert e.check_redzones() == 0
    e.close()


def test_another_kind_is_refused():
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_CARTPOLE, 2, max_members=2)
    with pytest.raises(_lib.DneError) as ei:
        e.mujoco_ga_reserve(2)
    assert str(ei.value) == "dne_mujoco_ga_reserve needs a DNE_KIND_PENDULUM or DNE_KIND_MJMAZE engine (this one: kind 5)"
    with pytest.raises(_lib.DneError, match="dne_mujoco_ga_parents needs a DNE_KIND_PENDULUM or DNE_KIND_MJMAZE engine"):
        e.mujoco_ga_parents()
    e.close()
