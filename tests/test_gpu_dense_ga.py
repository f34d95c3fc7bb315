"""GPU: Deep-GA on the dense kind (csrc/dense_ga.h) on a DNE_KIND_DENSE engine, BIT FOR BIT, on the five shapes of dense_ga_support.CASES
(P = 24, 256, 291, 498, 9218: the edges of the kernels' 256-wide blocks): k_dense_ga_build against the numpy genomes; dne_dense_ga_eval
(k_dense_ga_roots + k_dense_run over the bank) against dne_dense_rollout_host on dne_dense_ga_members_host's thetas at n = 1, 3, 5, 9 and
tslimit 1, 7 and the environment's own; the same descriptors on the baked kernels at (16, 16); k_dense_ga_promote with the aliasing cases,
and after three chained generations against dne_dense_ga_build of every parent's whole genome; what a GA call must not touch; every refusal
with the bank read back (host-side checks: nothing is launched); and ga_gpu.main on this engine against the same call on DenseGaHostEngine."""
import numpy as np
import pytest

import dense_ga_support as S
import dense_support as D
import maze_ga_support as MG
import maze_support as M
import stepenv_support as SS

pytestmark = pytest.mark.gpu

CASE_IDS = [S.case_id(c) for c in S.CASES]
SLOT0, SLOT1 = 11, 22                      # seeds of what the caller keeps in base slots 0 and 1
OWN = {"maze": 400, "cartpole": 500, "pendulum": 200}


def slot_theta(P, seed):
    return (np.random.RandomState(seed).randn(P) * 0.3).astype(np.float32)


@pytest.fixture(scope="module", params=S.CASES, ids=CASE_IDS)
def shaped(request):
    """(case, engine) of every shape: max_members 16, base slots 0 and 1 holding the caller's own vectors, which must survive the module"""
    case = request.param
    e = S.device_engine(case, 16)
    e.set_theta(slot_theta(e.P, SLOT0), 0)
    e.set_theta(slot_theta(e.P, SLOT1), 1)
    yield case, e
    assert same_bits(e.get_theta(0), slot_theta(e.P, SLOT0)) and same_bits(e.get_theta(1), slot_theta(e.P, SLOT1))
    assert e.check_redzones() == 0
    e.close()


def bank_of(eng):
    T = eng.dense_ga_parents()
    return np.stack([eng.dense_ga_get_parent(j) for j in range(T)]) if T else np.zeros((0, eng.P), np.float32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(SS.bits(a), SS.bits(b))


def numpy_bank(case, genomes):
    return np.stack([S.genome_theta(S.noise(), S.scale_by(case), g) for g in genomes])


# ---- build -----------------------------------------------------------------------------------------------------------------------------------------
def test_build_equals_the_numpy_genomes(shaped):
    case, eng = shaped
    genomes = S.genomes(eng.P) + S.bank_genomes(eng.P, 6)
    assert len(genomes) == 16 == eng.max_members                                                  # T = max_members is allowed
    eng.dense_ga_build(genomes)
    assert eng.dense_ga_parents() == 16 and same_bits(bank_of(eng), numpy_bank(case, genomes))     # every slot read back
    eng.dense_ga_build(genomes[3:4])                                                              # a smaller bank replaces it
    assert eng.dense_ga_parents() == 1 and same_bits(bank_of(eng), numpy_bank(case, genomes[3:4]))
    assert eng.check_redzones() == 0


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------------------
def eval_members(case, T, n):
    """n descriptors over a bank of T (roots, power-0 parents, children) and the seeds of their episodes.  On the cart-pole members 1 and
    n - 1 are one member under two seeds, seeds 3 and 4 one seed under two members, and the seeds are a window of the pool under which the
    twin's episodes end at three or more different steps"""
    P = S.num_params(case)
    parent, idx, power = S.eval_descriptors(P, T, n, seed=n)
    if case[0] == "maze":
        return parent, idx, power, None
    if n >= 5:
        parent[-1], idx[-1], power[-1] = parent[1], idx[1], power[1]
    pool = SS.mixed_seeds(64)
    seeds = pool[:n].copy()
    if case[0] == "cartpole" and n >= 5:
        bank = numpy_bank(case, S.bank_genomes(P, T)) if T else None
        thetas = S.members_theta(S.noise(), S.scale_by(case), bank, parent, idx, power)
        for k in range(64 - n):
            seeds = pool[k:k + n].copy()
            seeds[4] = seeds[3]
            if len(set(S.rollout(case, thetas, 0, seeds)["lengths"].tolist())) >= 3:
                break
        else:
            raise AssertionError("no window of the seed pool spreads the episode lengths")
        assert seeds[1] != seeds[n - 1] and (parent[3], idx[3], power[3]) != (parent[4], idx[4], power[4])
    return parent, idx, power, seeds


@pytest.mark.parametrize("T", (0, 3))
def test_eval_equals_the_host_episodes(shaped, T):
    from dne_hip import _lib
    case, eng = shaped
    sb = S.scale_by(case)
    if T:
        eng.dense_ga_build(S.bank_genomes(eng.P, T))
    else:                                                                                         # an empty bank: a fresh engine (generation 0)
        eng = S.device_engine(case, 9)
    try:
        bank = bank_of(eng)
        assert len(bank) == T
        for n in S.COUNTS:
            parent, idx, power, seeds = eval_members(case, T, n)
            assert T == 0 or n < 3 or ({"root", "again", "child"} ==
                                       {"root" if a < 0 else "again" if (b == 0 and c == 0) else "child" for a, b, c in zip(parent, idx, power)})
            thetas = _lib.dense_ga_members_host(S.noise(), sb, bank if T else None, parent, idx, power)
            for tslimit in (1, 7, OWN[case[0]]):
                ret, sg, ln = eng.dense_ga_eval(parent, idx, power, tslimit, seeds)
                want = S.rollout(case, thetas, tslimit, seeds)
                assert same_bits(ret, want["returns"]) and same_bits(sg, want["signreturns"]) and np.array_equal(ln, want["lengths"]), (T, n, tslimit)
                assert same_bits(eng.dense_final_state(n), want["state"]), (T, n, tslimit)
                prof = eng.profile()
                assert prof["env_steps"] == int(want["lengths"].sum()) and prof["eval_ms"] > 0
            if case[0] == "cartpole" and n >= 5:                                                  # (the last evaluation ran at the own limit)
                assert len(set(ln.tolist())) >= 3
        assert same_bits(bank_of(eng), bank)                                                      # an evaluation leaves the bank alone
        assert eng.check_redzones() == 0
    finally:
        if not T:
            eng.close()


def test_roots_with_signed_zero_biases_run_from_their_scratch_slots():
    """every bias of these roots is -0.0 or +0.0 by the noise's sign; the scratch slot at scale 0 keeps each bit (theta + fl(0 * eps))"""
    from dne_hip import _lib
    case = S.CASES[2]
    P = S.num_params(case)
    table = S.signed_zero_noise(P)
    env, hidden, nl = case
    e = _lib.Engine(_lib.KIND_DENSE, 2, max_members=4, env=SS.kind_id(env), hidden=hidden, nonlin=nl)
    try:
        e.noise_upload(table)
        e.dense_ga_set_init_scale(S.scale_by(case))
        parent, idx, power = np.full(3, -1, np.int32), np.array([0, P, table.size - P], np.int64), np.full(3, 1e30, np.float32)   # (a root's power is not read)
        seeds = SS.mixed_seeds(3)
        ret, sg, ln = e.dense_ga_eval(parent, idx, power, 500, seeds)
        want = S.rollout(case, _lib.dense_ga_members_host(table, S.scale_by(case), None, parent, idx, power), 500, seeds)
        assert same_bits(ret, want["returns"]) and np.array_equal(ln, want["lengths"]) and same_bits(e.dense_final_state(3), want["state"])
        e.dense_ga_promote(parent, idx, power)                                                    # the same roots as parents: their bits in the bank
        assert np.all(M.bits(bank_of(e)[0][S.bias_positions(case)]) == 0x80000000)
        assert same_bits(bank_of(e), _lib.dense_ga_members_host(table, S.scale_by(case), None, parent, idx, power))
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- the same descriptors on the baked kernels, at (16, 16) ---------------------------------------------------------------------------------------------
def test_maze_16_16_equals_maze_ga_eval_on_a_maze_handle():
    from dne_hip import _lib
    eng = S.device_engine(S.CASES[3], 16)
    baked = _lib.Engine(_lib.KIND_MAZE, 2, max_members=16)
    try:
        baked.noise_upload(S.noise()); baked.maze_set_walls(*M.fixture_maze()); baked.maze_ga_set_init_scale(MG.scale_by())
        genomes = S.bank_genomes(eng.P, 3)
        eng.dense_ga_build(genomes); baked.maze_ga_build(genomes)
        for j in range(3):
            assert same_bits(eng.dense_ga_get_parent(j), baked.maze_ga_get_parent(j))
        for n in S.COUNTS:
            parent, idx, power = S.eval_descriptors(eng.P, 3, n, seed=n)
            for tslimit in (7, 400):
                a = eng.dense_ga_eval(parent, idx, power, tslimit)
                b = baked.maze_ga_eval(parent, idx, power, tslimit)
                assert all(same_bits(x, y) for x, y in zip(a, b)), (n, tslimit)
        desc = S.descriptors(eng.P, 3, 5, seed=6, kept=True)
        eng.dense_ga_promote(*desc); baked.maze_ga_promote(*desc)
        for j in range(5):
            assert same_bits(eng.dense_ga_get_parent(j), baked.maze_ga_get_parent(j))
    finally:
        eng.close(); baked.close()


def test_cartpole_16_16_equals_eval_members_on_a_cartpole_handle():
    """the twin's thetas through base slots of a DNE_KIND_CARTPOLE handle (k_cartpole_rollout) against the same descriptors on the dense kind"""
    from dne_hip import _lib
    case = ("cartpole", (16, 16), "relu")
    eng = S.device_engine(case, 9)
    baked = _lib.Engine(_lib.KIND_CARTPOLE, 2, max_members=9)
    try:
        assert eng.P == baked.P == 386
        baked.noise_upload(S.noise())
        eng.dense_ga_build(S.bank_genomes(eng.P, 3))
        parent, idx, power = S.eval_descriptors(eng.P, 3, 9, seed=9)
        thetas = _lib.dense_ga_members_host(S.noise(), S.scale_by(case), bank_of(eng), parent, idx, power)
        for i, th in enumerate(thetas):
            baked.set_theta(th, i)
        baked.set_members(np.arange(9, dtype=np.int32), np.zeros(9, np.int64), np.zeros(9, np.float32))
        seeds = SS.mixed_seeds(9)
        for tslimit in (7, 500):
            a = eng.dense_ga_eval(parent, idx, power, tslimit, seeds)
            b = baked.eval_members(9, tslimit, seeds)
            assert all(same_bits(x, y) for x, y in zip(a, b)), tslimit
            assert same_bits(eng.dense_final_state(9), baked.cartpole_final_state(9))
    finally:
        eng.close(); baked.close()


# ---- promotion -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 3, 5))
def test_promote_equals_numpy_on_every_form_with_aliasing(shaped, T):
    case, eng = shaped
    sb = S.scale_by(case)
    for T_new in (1, 3, 5):
        eng.dense_ga_build(S.bank_genomes(eng.P, T))
        old = bank_of(eng)
        parent, idx, power = S.descriptors(eng.P, T, T_new, seed=T_new + 1, kept=True)
        eng.dense_ga_promote(parent, idx, power)
        assert eng.dense_ga_parents() == T_new
        assert same_bits(bank_of(eng), S.members_theta(S.noise(), sb, old, parent, idx, power)), (T, T_new, parent, idx)
        if T_new >= 2:
            assert parent[-1] == parent[-2] and idx[-1] < 0 and idx[-2] < 0                        # one source, twice
            assert same_bits(eng.dense_ga_get_parent(T_new - 1), old[parent[-1]]) and same_bits(eng.dense_ga_get_parent(T_new - 2), old[parent[-1]])


def test_three_chained_promotions_equal_build_of_the_whole_genomes(shaped):
    case, eng = shaped
    last = S.noise().size - eng.P
    genomes = S.bank_genomes(eng.P, 5)
    eng.dense_ga_build(genomes)
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
        eng.dense_ga_promote(parent, idx, power)
        genomes = nxt
    promoted = bank_of(eng)
    eng.dense_ga_build(genomes)
    assert max(len(g) for g in genomes) >= 12
    assert same_bits(promoted, bank_of(eng))
    assert same_bits(promoted, numpy_bank(case, genomes))
    assert eng.check_redzones() == 0


# ---- what a GA call must not touch -----------------------------------------------------------------------------------------------------------------------
def test_base_slots_set_members_and_the_step_batch_survive(shaped):
    case, eng = shaped
    env = case[0]
    members = (np.array([0, 1, 1], np.int32), np.array([5, 77, 0], np.int64), np.array([0.02, -0.02, 0.0], np.float32))
    seeds = SS.mixed_seeds(3)
    eng.set_members(*members)
    before = eng.eval_members(3, 50, seeds)
    eng.stepenv_reset(n=4, seeds=SS.mixed_seeds(4), max_steps=9)
    eng.stepenv_run(2, indices=[0, 1, 2], members=[0, 1, 2])
    batch = eng.stepenv_state(n=4)
    obs = eng.stepenv_observation(n=4)
    eng.dense_ga_build(S.bank_genomes(eng.P, 3))
    eng.dense_ga_eval(*S.eval_descriptors(eng.P, 3, 9, seed=2), tslimit=7, env_seed=None if env == "maze" else SS.mixed_seeds(9))
    eng.dense_ga_promote(*S.descriptors(eng.P, 3, 5, seed=3, kept=True))
    for slot, seed in ((0, SLOT0), (1, SLOT1)):
        assert same_bits(eng.get_theta(slot), slot_theta(eng.P, seed))
    assert all(same_bits(a, b) for a, b in zip(batch, eng.stepenv_state(n=4))) and same_bits(obs, eng.stepenv_observation(n=4))
    after = eng.eval_members(3, 50, seeds)                                                        # dne_set_members' descriptors are their own
    assert all(same_bits(a, b) for a, b in zip(before, after))
    base = {0: slot_theta(eng.P, SLOT0), 1: slot_theta(eng.P, SLOT1)}
    want = S.rollout(case, np.stack([S.perturbed(base[int(s)], S.noise(), int(o), c) for s, o, c in zip(*members)]), 50, seeds)
    assert same_bits(after[0], want["returns"]) and np.array_equal(after[2], want["lengths"])
    r1 = eng.stepenv_run(3, indices=[0, 1, 2], members=[0, 1, 2])                                 # the step batch goes on with dne_set_members' members
    assert np.array_equal(eng.stepenv_state(n=4)[1][:3], batch[1][:3] + r1[1])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_bank_as_it_was(shaped):
    from dne_hip import _lib
    case, eng = shaped
    P, last = eng.P, S.noise().size - eng.P
    seeds = None if case[0] == "maze" else np.zeros(17, np.uint32)
    ev = lambda parent, idx, power, tslimit=7: eng.dense_ga_eval(parent, idx, power, tslimit, None if seeds is None else seeds[:len(parent)])
    eng.dense_ga_build(S.bank_genomes(P, 3))
    bank = bank_of(eng)
    z = lambda n: np.zeros(n, np.float32)
    refused = [
        (lambda: ev([3], [0], z(1)), "dne_dense_ga_eval: member 0: parent 3, the bank holds 3"),
        (lambda: ev([0, -2], [0, 0], z(2)), "member 1: parent -2"),
        (lambda: ev([0], [-1], z(1)), "kept form .* is for promotion only"),
        (lambda: ev([-1], [-1], z(1)), "a root needs a noise index"),
        (lambda: ev([0], [last + 1], z(1)), r"noise index %d \+ P = %d outside the table of %d" % (last + 1, P, S.noise().size)),
        (lambda: ev([-1], [last + 1], z(1)), r"\+ P = %d outside the table" % P),
        (lambda: ev([], [], z(0)), r"n = 0 outside \[1, max_members = 16\]"),
        (lambda: ev([0] * 17, [0] * 17, z(17)), "n = 17 outside"),
        (lambda: ev([0], [0], z(1), 0), "dne_dense_ga_eval: timestep limit must be positive"),
        (lambda: ev([0], [0], z(1), -3), "timestep limit must be positive"),
        (lambda: eng.dense_ga_promote([3], [0], z(1)), "dne_dense_ga_promote: member 0: parent 3, the bank holds 3"),
        (lambda: eng.dense_ga_promote([0, 1], [0, last + 1], z(2)), "member 1: noise index"),
        (lambda: eng.dense_ga_promote([-1], [-3], z(1)), "a root needs a noise index"),
        (lambda: eng.dense_ga_promote([], [], z(0)), "T = 0 outside"),
        (lambda: eng.dense_ga_promote([0] * 17, [0] * 17, z(17)), "T = 17 outside"),
        (lambda: eng.dense_ga_build([]), "T = 0 outside"),
        (lambda: eng.dense_ga_build([(0, )] * 17), "T = 17 outside"),
        (lambda: eng.dense_ga_build([(0, ), ()]), "genome 1: empty chain"),
        (lambda: eng.dense_ga_build([(0, (last + 1, 0.1))]), r"genome 0: noise index %d \+ P = %d" % (last + 1, P)),
        (lambda: eng.dense_ga_build([(-1, )]), "genome 0: noise index -1"),
        (lambda: eng.dense_ga_get_parent(3), "parent 3, the bank holds 3"),
        (lambda: eng.dense_ga_get_parent(-1), "parent -1, the bank holds 3"),
        (lambda: eng.dense_ga_set_init_scale(np.zeros(P - 1, np.float32)), "expected P = %d values, got %d" % (P, P - 1)),
    ]
    if case[0] != "maze":
        refused.append((lambda: eng.dense_ga_eval([0], [0], z(1), 7, None), "dne_dense_ga_eval: a DNE_KIND_DENSE engine on the .* env_seed is NULL"))
    for call, text in refused:
        with pytest.raises(_lib.DneError, match=text):
            call()
        assert eng.dense_ga_parents() == 3 and same_bits(bank_of(eng), bank), text
    # the raw entry points: chain_offsets[0] != 0, a missing buffer
    import ctypes as C
    co, sd, pw = np.array([1, 2], np.int32), np.zeros(2, np.int64), np.zeros(2, np.float32)
    ip, lp, fp = co.ctypes.data_as(C.POINTER(C.c_int32)), sd.ctypes.data_as(C.POINTER(C.c_int64)), pw.ctypes.data_as(C.POINTER(C.c_float))
    for call, text in ((lambda: eng.lib.dne_dense_ga_build(eng.h, 1, ip, lp, fp), b"dne_dense_ga_build: chain_offsets starts at 1, not 0"),
                       (lambda: eng.lib.dne_dense_ga_build(eng.h, 1, ip, None, fp), b"dne_dense_ga_build: a buffer is missing"),
                       (lambda: eng.lib.dne_dense_ga_promote(eng.h, 1, ip, lp, None), b"dne_dense_ga_promote: a buffer is missing"),
                       (lambda: eng.lib.dne_dense_ga_eval(eng.h, 1, ip, lp, fp, None, 7, None, None, ip), b"dne_dense_ga_eval: a buffer is missing"),
                       (lambda: eng.lib.dne_dense_ga_get_parent(eng.h, 0, None), b"dne_dense_ga_get_parent: no output buffer")):
        assert call() == -1 and text in eng.lib.dne_last_error(eng.h)
        assert eng.dense_ga_parents() == 3 and same_bits(bank_of(eng), bank), text
    # the maze's own bank and archive keep refusing the kind, in their words
    with pytest.raises(_lib.DneError, match=r"dne_maze_ga_build needs a DNE_KIND_MAZE engine \(this one: kind 8\)"):
        eng.maze_ga_build([(0, )])
    with pytest.raises(_lib.DneError, match=r"dne_maze_ga_eval needs a DNE_KIND_MAZE engine \(this one: kind 8\)"):
        eng.maze_ga_eval([-1], [0], z(1))
    assert same_bits(bank_of(eng), bank)


def test_refusals_of_an_unprepared_engine_and_of_another_kind():
    from dne_hip import _lib
    z = np.zeros(1, np.float32)

    def fresh(case, noise=True, walls=True, scale=True):
        env, hidden, nl = case
        e = _lib.Engine(_lib.KIND_DENSE, D.N_OUT[env], max_members=4, env=SS.kind_id(env), hidden=hidden, nonlin=nl)
        if noise:
            e.noise_upload(S.noise())
        if walls and env == "maze":
            e.maze_set_walls(*M.fixture_maze())
        if scale:
            e.dense_ga_set_init_scale(S.scale_by(case))
        return e

    maze, cart = S.CASES[0], S.CASES[2]
    for case, kw, text, evals_only in ((maze, dict(scale=False), "no init scale", False), (cart, dict(noise=False), "noise table not uploaded", False),
                                       (maze, dict(walls=False), "no maze loaded", True)):
        e = fresh(case, **kw)
        seeds = None if case[0] == "maze" else np.zeros(1, np.uint32)
        try:
            with pytest.raises(_lib.DneError, match="dne_dense_ga_eval: " + text):
                e.dense_ga_eval([-1], [0], z, 7, seeds)
            if not evals_only:
                with pytest.raises(_lib.DneError, match="dne_dense_ga_build: " + text):
                    e.dense_ga_build([(0, )])
                with pytest.raises(_lib.DneError, match="dne_dense_ga_promote: " + text):
                    e.dense_ga_promote([-1], [0], z)
                assert e.dense_ga_parents() == 0
            else:                                                                                 # the bank needs no walls
                e.dense_ga_build([(0, )])
                e.dense_ga_promote([0, -1], [-1, 5], [0.0, 0.0])
                assert e.dense_ga_parents() == 2
        finally:
            e.close()
    e = fresh(cart)
    try:
        for call in (lambda: e.dense_ga_eval([0], [0], z, 7, np.zeros(1, np.uint32)), lambda: e.dense_ga_promote([0], [0], z),
                     lambda: e.dense_ga_promote([0], [-1], z)):
            with pytest.raises(_lib.DneError, match="parent 0 on an empty bank"):
                call()
        assert e.dense_ga_parents() == 0
    finally:
        e.close()
    other = _lib.Engine(_lib.KIND_MAZE, 2, max_members=4)
    try:
        calls = {
            "dne_dense_ga_set_init_scale": lambda: other.dense_ga_set_init_scale(MG.scale_by()),
            "dne_dense_ga_build": lambda: other.dense_ga_build([(0, )]),
            "dne_dense_ga_eval": lambda: other.dense_ga_eval([-1], [0], z, 7),
            "dne_dense_ga_promote": lambda: other.dense_ga_promote([-1], [0], z),
            "dne_dense_ga_parents": lambda: other.dense_ga_parents(),
            "dne_dense_ga_get_parent": lambda: other.dense_ga_get_parent(0),
        }
        for name, call in calls.items():
            with pytest.raises(_lib.DneError, match=name + r" needs a DNE_KIND_DENSE engine \(this one: kind 4\)"):
                call()
    finally:
        other.close()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------------------
def _same_run(a, b):
    (ta, va, sa), (tb, vb, sb) = a, b
    ok = (ta, va) == (tb, vb) and sa.it == sb.it and [o.seeds for o in sa.population] == [o.seeds for o in sb.population]
    ok = ok and [o.rewards for o in sa.population] == [o.rewards for o in sb.population] and sa.elite.seeds == sb.elite.seeds
    return ok and (sa.curr_solution, sa.timesteps_so_far, sa.num_frames) == (sb.curr_solution, sb.timesteps_so_far, sb.num_frames)


DRIVER = {"linear-maze": ("maze", "LinearClassifier", ("maze", (), "relu")),
          "linear-cartpole": ("gym.CartPole-v1", "LinearClassifier", ("cartpole", (), "relu")),
          "simple-cartpole": ("gym.CartPole-v1", None, ("cartpole", (16, 16), "relu"))}


@pytest.mark.parametrize("config", sorted(DRIVER))
def test_driver_on_the_hip_engine_equals_the_host_engine(oracle, tmp_path, config):
    from dne_hip import ga_gpu
    game, model, case = DRIVER[config]
    exp = S.exp(game, model=model)
    hip, host = D.device_engine(case, 10), S.host_engine(case, 10)
    try:
        hip.set_theta(slot_theta(hip.P, SLOT0), 0)
        for it in (2, 4):                                                                         # the second round resumes, on each side
            a = ga_gpu.main(str(tmp_path / "hip"), engine=hip, noise=S.shared_noise(), seed=4, max_iters=2, **exp)
            b = ga_gpu.main(str(tmp_path / "host"), engine=host, noise=S.shared_noise(), seed=4, max_iters=2, **exp)
            assert a[2].it == it and _same_run(a, b) and same_bits(bank_of(hip), host.bank)
        assert D.log_rows(tmp_path / "hip") == D.log_rows(tmp_path / "host")
        assert same_bits(hip.get_theta(0), slot_theta(hip.P, SLOT0)) and hip.check_redzones() == 0
    finally:
        hip.close()


@pytest.mark.parametrize("config", sorted(DRIVER))
def test_driver_builds_its_own_engine(oracle, tmp_path, config):
    from dne_hip import ga_gpu
    game, model, case = DRIVER[config]
    exp = S.exp(game, model=model or "SimpleClassifier")
    a = ga_gpu.main(str(tmp_path / "own"), noise=S.shared_noise(), seed=4, max_iters=3, **exp)
    b = ga_gpu.main(str(tmp_path / "host"), engine=S.host_engine(case, 10), noise=S.shared_noise(), seed=4, max_iters=3, **dict(exp, model=model))
    assert a[2].it == 3 and _same_run(a, b) and (a[2].model, a[2].num_params) == (exp["model"], S.num_params(case))


def test_driver_at_16_16_on_the_maze_equals_maze_main_on_a_maze_handle(oracle, tmp_path):
    from dne_hip import _lib, ga_gpu
    dense, baked = D.device_engine(S.CASES[3], 10), _lib.Engine(_lib.KIND_MAZE, 2, max_members=10)
    try:
        a = ga_gpu.main(str(tmp_path / "dense"), engine=dense, noise=S.shared_noise(), seed=4, max_iters=4, **S.exp("maze", model=None))
        b = ga_gpu.main(str(tmp_path / "maze"), engine=baked, noise=S.shared_noise(), seed=4, max_iters=4, **S.exp("maze", model="SimpleClassifier"))
        assert a[2].it == 4 and _same_run(a, b) and D.log_rows(tmp_path / "dense") == D.log_rows(tmp_path / "maze")
        assert dense.dense_ga_parents() == baked.maze_ga_parents() == 3
        for j in range(3):
            assert same_bits(dense.dense_ga_get_parent(j), baked.maze_ga_get_parent(j))
    finally:
        dense.close(); baked.close()
