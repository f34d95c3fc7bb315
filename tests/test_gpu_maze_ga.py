"""GPU: Deep-GA on the hard maze (csrc/maze_ga.h) on a DNE_KIND_MAZE engine, BIT FOR BIT: k_maze_ga_build against the numpy genomes of
tests/test_maze_ga_cpu.py; dne_maze_ga_eval (k_maze_ga_roots + k_maze_rollout over the bank) against dne_maze_rollout_host on
dne_maze_ga_members_host's thetas, at member counts 1, 3, 4, 5, 9; k_maze_ga_promote with the aliasing cases, and after three chained
generations against dne_maze_ga_build of every parent's whole genome; the caller's base slots; every refusal with the bank read back;
and dne_hip/ga_gpu.py's maze loop on this engine against the same loop on MazeGaHostEngine."""
import numpy as np
import pytest

import maze_ga_support as S
import maze_support as M

pytestmark = pytest.mark.gpu

SLOT0, SLOT1 = 11, 22                      # seeds of what the caller keeps in base slots 0 and 1


def slot_theta(seed):
    return np.random.RandomState(seed).randn(S.P).astype(np.float32)


def fresh(max_members=16, walls=True, noise=True, scale=True):
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_MAZE, 2, max_members=max_members)
    if noise:
        e.noise_upload(S.noise())
    if walls:
        e.maze_set_walls(*M.fixture_maze())
    if scale:
        e.maze_ga_set_init_scale(S.scale_by())
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


def bank_of(eng):
    return np.stack([eng.maze_ga_get_parent(j) for j in range(eng.maze_ga_parents())]) if eng.maze_ga_parents() else np.zeros((0, S.P), np.float32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(M.bits(a), M.bits(b))


# ---- build -----------------------------------------------------------------------------------------------------------------------------------------
def test_build_equals_the_numpy_genomes(eng):
    genomes = list(S.genomes())
    assert len(genomes) == 16 == eng.max_members                                                  # T = max_members is allowed
    eng.maze_ga_build(genomes)
    assert eng.maze_ga_parents() == 16 and same_bits(bank_of(eng), S.genome_thetas())
    eng.maze_ga_build(genomes[3:4])                                                               # a smaller bank replaces it
    assert eng.maze_ga_parents() == 1 and same_bits(bank_of(eng), S.genome_thetas()[3:4])
    assert eng.check_redzones() == 0


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------------------
def host_episodes(bank, parent, idx, power, maze, tslimit):
    from dne_hip import _lib
    thetas = _lib.maze_ga_members_host(S.noise(), S.scale_by(), bank if len(bank) else None, parent, idx, power)
    return _lib.maze_rollout_host(thetas, maze[0], maze[1], tslimit)


@pytest.mark.parametrize("maze_name", ("fixture", "one_wall"))
@pytest.mark.parametrize("T", S.BANKS)
def test_eval_equals_the_host_episodes(eng, maze_name, T):
    maze = M.fixture_maze() if maze_name == "fixture" else M.synthetic_maze(1)
    eng.maze_set_walls(*maze)
    eng.maze_ga_build(S.bank_genomes(T))
    bank = bank_of(eng)
    for n in S.COUNTS:
        parent, idx, power = S.descriptors(T, n, seed=n)
        for tslimit in (400, 37):
            ret, sg, ln = eng.maze_ga_eval(parent, idx, power, tslimit)
            want_ret, want_ln, want_xy = host_episodes(bank, parent, idx, power, maze, tslimit)
            assert same_bits(ret, want_ret) and np.array_equal(ln, want_ln) and np.array_equal(sg, np.sign(want_ret)), (T, n, tslimit)
            assert same_bits(eng.maze_final_state(n), want_xy), (T, n, tslimit)
    prof = eng.profile()                                                                          # the last evaluation: nine members, 37 steps each
    assert prof["env_steps"] == 9 * 37 and prof["eval_ms"] > 0
    assert same_bits(bank_of(eng), bank)                                                          # an evaluation leaves the bank alone
    eng.maze_set_walls(*M.fixture_maze())
    assert eng.check_redzones() == 0


def test_eval_of_roots_alone_on_an_empty_bank_and_what_follows_an_evaluation():
    """no parents yet (generation 0): every member a root, in its scratch slot at scale 0 -- signed-zero biases included"""
    from dne_hip import _lib
    e = fresh(max_members=9, noise=False)
    try:
        noise = S.signed_zero_noise()
        e.noise_upload(noise)
        assert e.maze_ga_parents() == 0
        maze = M.fixture_maze()
        for n in S.COUNTS:
            idx = np.array(([0, S.P, noise.size - S.P] + [int(v) for v in np.random.RandomState(n).randint(0, noise.size - S.P + 1, size=n)])[:n], np.int64)
            parent, power = np.full(n, -1, np.int32), np.full(n, 1e30, np.float32)                 # (a root's power is not read)
            ret, sg, ln = e.maze_ga_eval(parent, idx, power)
            thetas = _lib.maze_ga_members_host(noise, S.scale_by(), None, parent, idx, power)
            want_ret, want_ln, want_xy = _lib.maze_rollout_host(thetas, maze[0], maze[1], 400)
            assert same_bits(ret, want_ret) and np.array_equal(ln, want_ln) and same_bits(e.maze_final_state(n), want_xy), n
        # dne_maze_novelty(xy = NULL) and the archive's device-to-device append follow it as they follow any evaluation
        e.maze_archive_append(n=9)
        assert same_bits(e.maze_archive(), want_xy)
        assert np.array_equal(e.maze_novelty(2, n=9), _lib.maze_novelty_host(want_xy, want_xy, 2))
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- promotion -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", S.BANKS)
@pytest.mark.parametrize("T_new", S.BANKS)
def test_promote_equals_numpy_on_every_form_with_aliasing(eng, T, T_new):
    eng.maze_ga_build(S.bank_genomes(T))
    old = bank_of(eng)
    parent, idx, power = S.descriptors(T, T_new, seed=T_new + 1, kept=True)
    eng.maze_ga_promote(parent, idx, power)
    assert eng.maze_ga_parents() == T_new
    assert same_bits(bank_of(eng), S.members_theta(S.noise(), old, parent, idx, power)), (T, T_new, parent, idx)
    if T_new >= 2:
        assert parent[-1] == parent[-2] and idx[-1] < 0 and idx[-2] < 0                            # one source, twice
        assert same_bits(eng.maze_ga_get_parent(T_new - 1), old[parent[-1]]) and same_bits(eng.maze_ga_get_parent(T_new - 2), old[parent[-1]])


def test_three_chained_promotions_equal_build_of_the_whole_genomes(eng):
    last = S.noise().size - S.P
    genomes = S.bank_genomes(5)
    eng.maze_ga_build(genomes)
    rs = np.random.RandomState(321)
    for gen in range(3):
        T_new = (5, 3, 5)[gen]
        parent = rs.randint(len(genomes), size=T_new).astype(np.int32)
        idx = rs.randint(0, last + 1, size=T_new).astype(np.int64)
        power = np.array([S.POWERS[(j + gen) % len(S.POWERS)] for j in range(T_new)], np.float32)
        idx[0] = (0, last, -1)[gen]                                                               # the table's ends; in the last generation a kept parent ...
        if gen == 2:
            parent[0], parent[1], idx[1] = 2, 2, -5                                               # ... that moves from index 2 to 0 and 1
        if gen == 1:
            parent[2] = -1                                                                        # a fresh root among the promoted
        nxt = []
        for a, b, c in zip(parent, idx, power):
            nxt.append((int(b), ) if a < 0 else genomes[a] if b < 0 else tuple(genomes[a]) + ((int(b), float(c)), ))
        eng.maze_ga_promote(parent, idx, power)
        genomes = nxt
    promoted = bank_of(eng)
    eng.maze_ga_build(genomes)
    assert max(len(g) for g in genomes) >= 12
    assert same_bits(promoted, bank_of(eng))
    assert same_bits(promoted, np.stack([S.genome_theta(S.noise(), g) for g in genomes]))
    assert eng.check_redzones() == 0


# ---- the caller's base slots --------------------------------------------------------------------------------------------------------------------------
def test_base_slots_survive_and_set_members_evaluations_are_untouched(eng):
    from dne_hip import _lib
    maze = M.fixture_maze()
    members = (np.array([0, 1, 1], np.int32), np.array([5, 77, 0], np.int64), np.array([0.02, -0.02, 0.0], np.float32))
    eng.set_members(*members)
    before = eng.eval_members(3, 400, np.zeros(3, np.uint32))
    eng.maze_ga_build(S.bank_genomes(3))
    eng.maze_ga_eval(*S.descriptors(3, 9, seed=2))
    eng.maze_ga_promote(*S.descriptors(3, 5, seed=3, kept=True))
    for slot, seed in ((0, SLOT0), (1, SLOT1)):
        assert same_bits(eng.get_theta(slot), slot_theta(seed))
    after = eng.eval_members(3, 400, np.zeros(3, np.uint32))                                      # dne_set_members' descriptors are their own
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    base = {0: slot_theta(SLOT0), 1: slot_theta(SLOT1)}
    want = _lib.maze_rollout_host(np.stack([M.perturbed(base[int(s)], S.noise(), int(o), c) for s, o, c in zip(*members)]), maze[0], maze[1], 400)
    assert same_bits(after[0], want[0])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_bank_as_it_was(eng):
    from dne_hip import _lib
    last = S.noise().size - S.P
    eng.maze_ga_build(S.bank_genomes(3))
    bank = bank_of(eng)
    z = lambda n: np.zeros(n, np.float32)
    refused = [
        (lambda: eng.maze_ga_eval([3], [0], z(1)), "dne_maze_ga_eval: member 0: parent 3, the bank holds 3"),
        (lambda: eng.maze_ga_eval([0, -2], [0, 0], z(2)), "member 1: parent -2"),
        (lambda: eng.maze_ga_eval([0], [-1], z(1)), "kept form .* is for promotion only"),
        (lambda: eng.maze_ga_eval([-1], [-1], z(1)), "a root needs a noise index"),
        (lambda: eng.maze_ga_eval([0], [last + 1], z(1)), r"noise index %d \+ 498 outside the table" % (last + 1)),
        (lambda: eng.maze_ga_eval([-1], [last + 1], z(1)), "outside the table"),
        (lambda: eng.maze_ga_eval([], [], z(0)), r"n = 0 outside \[1, max_members = 16\]"),
        (lambda: eng.maze_ga_eval([0] * 17, [0] * 17, z(17)), "n = 17 outside"),
        (lambda: eng.maze_ga_eval([0], [0], z(1), 0), "timestep limit"),
        (lambda: eng.maze_ga_promote([3], [0], z(1)), "dne_maze_ga_promote: member 0: parent 3, the bank holds 3"),
        (lambda: eng.maze_ga_promote([0, 1], [0, last + 1], z(2)), "member 1: noise index"),
        (lambda: eng.maze_ga_promote([-1], [-3], z(1)), "a root needs a noise index"),
        (lambda: eng.maze_ga_promote([], [], z(0)), "T = 0 outside"),
        (lambda: eng.maze_ga_promote([0] * 17, [0] * 17, z(17)), "T = 17 outside"),
        (lambda: eng.maze_ga_build([]), "T = 0 outside"),
        (lambda: eng.maze_ga_build([(0, )] * 17), "T = 17 outside"),
        (lambda: eng.maze_ga_build([(0, ), ()]), "genome 1: empty chain"),
        (lambda: eng.maze_ga_build([(0, (last + 1, 0.1))]), "genome 0: noise index"),
        (lambda: eng.maze_ga_build([(-1, )]), "genome 0: noise index -1"),
        (lambda: eng.maze_ga_get_parent(3), "parent 3, the bank holds 3"),
        (lambda: eng.maze_ga_set_init_scale(np.zeros(497, np.float32)), "expected 498 values, got 497"),
    ]
    for call, text in refused:
        with pytest.raises(_lib.DneError, match=text):
            call()
        assert eng.maze_ga_parents() == 3 and same_bits(bank_of(eng), bank), text
    # the Atari genome store keeps refusing the kind
    with pytest.raises(_lib.DneError, match="dne_ga_set_init_scale is not available on a DNE_KIND_MAZE engine"):
        eng.ga_set_init_scale(S.scale_by())
    with pytest.raises(_lib.DneError, match="dne_ga_eval_powers is not available on a DNE_KIND_MAZE engine"):
        eng.ga_eval_powers([((1,), (2, 0.1))], 10, np.zeros(1, np.uint32))
    assert same_bits(bank_of(eng), bank)


def test_refusals_of_an_unprepared_engine_and_of_another_kind():
    from dne_hip import _lib
    z = np.zeros(1, np.float32)
    for kw, text, evals_only in ((dict(scale=False), "no init scale", False), (dict(noise=False), "noise table not uploaded", False),
                                 (dict(walls=False), "no maze loaded", True)):
        e = fresh(max_members=4, **kw)
        try:
            with pytest.raises(_lib.DneError, match="dne_maze_ga_eval: " + text):
                e.maze_ga_eval([-1], [0], z)
            if not evals_only:
                with pytest.raises(_lib.DneError, match="dne_maze_ga_build: " + text):
                    e.maze_ga_build([(0, )])
                with pytest.raises(_lib.DneError, match="dne_maze_ga_promote: " + text):
                    e.maze_ga_promote([-1], [0], z)
            else:                                                                                 # the bank needs no walls
                e.maze_ga_build([(0, )])
                e.maze_ga_promote([0, -1], [-1, 5], [0.0, 0.0])
                assert e.maze_ga_parents() == 2
        finally:
            e.close()
    e = fresh(max_members=4)
    try:
        for call in (lambda: e.maze_ga_eval([0], [0], z), lambda: e.maze_ga_promote([0], [0], z), lambda: e.maze_ga_promote([0], [-1], z)):
            with pytest.raises(_lib.DneError, match="parent 0 on an empty bank"):
                call()
        assert e.maze_ga_parents() == 0
    finally:
        e.close()
    other = _lib.Engine(_lib.KIND_GA, 18, max_members=4)
    try:
        calls = {
            "dne_maze_ga_set_init_scale": lambda: other.maze_ga_set_init_scale(S.scale_by()),
            "dne_maze_ga_build": lambda: other.maze_ga_build([(0, )]),
            "dne_maze_ga_eval": lambda: other.maze_ga_eval([-1], [0], z),
            "dne_maze_ga_promote": lambda: other.maze_ga_promote([-1], [0], z),
            "dne_maze_ga_parents": lambda: other.maze_ga_parents(),
            "dne_maze_ga_get_parent": lambda: other.maze_ga_get_parent(0),
        }
        for name, call in calls.items():
            with pytest.raises(_lib.DneError, match=name + r" needs a DNE_KIND_MAZE engine \(this one: kind 1\)"):
                call()
    finally:
        other.close()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------------
def _table():
    from dne_hip import es
    t = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    t.noise, t._engines = S.noise(), []
    return t


def _exp(**over):
    exp = {"game": "maze", "model": "SimpleClassifier", "population_size": 10, "selection_threshold": 3, "validation_threshold": 2,
           "num_validation_episodes": 2, "num_test_episodes": 2, "episode_cutoff_mode": 40, "mutation_power": 0.005, "timesteps": 10 ** 9,
           "maze_file": M.MAZE_FILE}
    exp.update(over)
    return exp


CONFIGS = {"plain": {}, "no_parents": {"selection_threshold": 0}, "wide_validation": {"validation_threshold": 4, "episode_cutoff_mode": 400}}


def _same_run(a, b):
    (ta, va, sa), (tb, vb, sb) = a, b
    ok = (ta, va) == (tb, vb) and sa.it == sb.it and [o.seeds for o in sa.population] == [o.seeds for o in sb.population]
    ok = ok and [o.rewards for o in sa.population] == [o.rewards for o in sb.population] and sa.elite.seeds == sb.elite.seeds
    return ok and (sa.curr_solution, sa.timesteps_so_far, sa.num_frames) == (sb.curr_solution, sb.timesteps_so_far, sb.num_frames)


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_driver_on_the_hip_engine_equals_the_host_engine(oracle, tmp_path, config):
    from dne_hip import ga_gpu
    over = CONFIGS[config]
    hip, host = fresh(max_members=10, walls=False, noise=False, scale=False), S.MazeGaHostEngine(max_members=10)
    try:
        hip.set_theta(slot_theta(SLOT0), 0)
        a = ga_gpu.main(str(tmp_path / "hip"), engine=hip, noise=_table(), seed=4, max_iters=2, **_exp(**over))
        b = ga_gpu.main(str(tmp_path / "host"), engine=host, noise=_table(), seed=4, max_iters=2, **_exp(**over))
        assert _same_run(a, b) and same_bits(bank_of(hip), host.bank)
        a = ga_gpu.main(str(tmp_path / "hip"), engine=hip, noise=_table(), seed=4, max_iters=2, **_exp(**over))       # resumed, on each side
        b = ga_gpu.main(str(tmp_path / "host"), engine=host, noise=_table(), seed=4, max_iters=2, **_exp(**over))
        assert a[2].it == 4 and _same_run(a, b) and same_bits(bank_of(hip), host.bank)
        assert same_bits(hip.get_theta(0), slot_theta(SLOT0)) and hip.check_redzones() == 0
    finally:
        hip.close()


def test_driver_builds_its_own_engine(oracle, tmp_path):
    from dne_hip import ga_gpu
    a = ga_gpu.main(str(tmp_path / "own"), noise=_table(), seed=4, max_iters=3, **_exp())
    b = ga_gpu.main(str(tmp_path / "host"), engine=S.MazeGaHostEngine(max_members=10), noise=_table(), seed=4, max_iters=3, **_exp())
    assert a[2].it == 3 and _same_run(a, b)
