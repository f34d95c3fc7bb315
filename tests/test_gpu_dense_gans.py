"""GPU: GA-NS on the dense kind (csrc/dense_novelty.h's pool form on a DNE_KIND_DENSE engine), BIT FOR BIT:
k_dense_novelty_pool<2> and <4> against the CPU twin on the grid, the lattice, random and edge sets and, for D = 2, against
k_maze_novelty_pool of a DNE_KIND_MAZE handle; the NULL form behind every kind of evaluation; k_dense_archive_gather in order, reversed,
repeated and across two reallocations; what the new calls leave alone; every refusal with the archive read back; and ga_gpu.dense_ns_main on
live handles against the same driver on DenseGaNsHostEngine and, at (16, 16) on the maze, against maze_ns_main on a DNE_KIND_MAZE handle."""
import ctypes as C

import numpy as np
import pytest

import dense_ga_support as G
import dense_gans_support as S
import dense_support as D
import stepenv_support as SS

pytestmark = pytest.mark.gpu

LINEAR = {2: ("maze", (), "relu"), 4: ("cartpole", (), "relu")}
NULL_CASES = (("maze", (), "relu"), ("cartpole", (5, 33), "relu"), ("pendulum", (64,), "tanh"))
OWN = {"maze": 400, "cartpole": 500, "pendulum": 200}


@pytest.fixture(scope="module")
def handles():
    """one live handle per D (no hidden layer, 16 members) for the calls that take their points from the host"""
    es = {dim: G.device_engine(case, 16) for dim, case in LINEAR.items()}
    yield es
    for e in es.values():
        assert e.check_redzones() == 0
        e.close()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(SS.bits(a), SS.bits(b))


def load(e, archive):
    e.dense_archive_clear()
    if len(archive):
        e.dense_archive_append(archive)
    assert e.dense_archive_size() == len(archive)


# ---- 1. the kernel against the twin, and against k_maze_novelty_pool -----------------------------------------------------------------------------------
def test_shapes_are_the_ones_asked_for():
    assert S.GPU_ARCHIVES == (0, 1, 63, 64, 65, 1020, 1024, 1025) and S.COUNTS == (1, 2, 3, 4, 5, 9) and S.KS == (1, 2, 25, 32) and S.TILE == 1024


@pytest.mark.parametrize("dim", S.DIMS)
@pytest.mark.parametrize("name", S.SETS)
def test_kernel_equals_the_twin_on_every_shape(handles, name, dim):
    from dne_hip import _lib
    e = handles[dim]
    assert e.dense_bc_dim() == dim
    for A in S.GPU_ARCHIVES:
        mem, arch = S.cell(name, dim, A, 9)
        load(e, arch)
        for n in S.COUNTS:
            if A + n - 1 < 1:
                continue
            for k in S.KS:
                want = _lib.dense_novelty_pool_host(mem[:n], arch, k)
                got = e.dense_novelty_pool(k, mem[:n])
                assert got.dtype == np.float64 and got.shape == (n, ) and S.same(got, want), (name, dim, A, n, k, got, want)
        assert e.dense_novelty_last_ms() > 0 and same_bits(e.dense_archive(), arch)


@pytest.mark.parametrize("dim", S.DIMS)
def test_kernel_equals_the_twin_on_the_edge_inputs(handles, dim):
    from dne_hip import _lib
    e = handles[dim]
    for name, (bc, archive, ks) in sorted(S.edge_cases(dim).items()):
        load(e, archive)
        for k in ks:
            for n in sorted(set(min(n, len(bc)) for n in S.COUNTS)):
                if len(archive) + n - 1 < 1:
                    continue
                got, want = e.dense_novelty_pool(k, bc[:n]), _lib.dense_novelty_pool_host(bc[:n], archive, k)
                assert S.same(got, want), (name, dim, k, n, got, want)


def test_two_coordinates_equal_k_maze_novelty_pool(handles):
    from dne_hip import _lib
    e = handles[2]
    mz = _lib.Engine(_lib.KIND_MAZE, 2, max_members=16)
    try:
        for name in S.SETS:
            for A in (0, 1, 65, 1020, 1024, 1025):
                mem, arch = S.cell(name, 2, A, 9)
                load(e, arch)
                mz.maze_archive_clear()
                if A:
                    mz.maze_archive_append(arch)
                for n in (2, 4, 9):
                    for k in S.KS:
                        assert S.same(e.dense_novelty_pool(k, mem[:n]), mz.maze_novelty_pool(k, mem[:n])), (name, A, n, k)
        for name, (bc, archive, ks) in sorted(S.edge_cases(2).items()):
            load(e, archive)
            mz.maze_archive_clear()
            if len(archive):
                mz.maze_archive_append(archive)
            for k in ks:
                assert S.same(e.dense_novelty_pool(k, bc), mz.maze_novelty_pool(k, bc)), (name, k)
    finally:
        mz.close()


# ---- 2. the NULL form behind every kind of evaluation ---------------------------------------------------------------------------------------------------
def e_members(case, extra):
    env, hidden, _ = case
    slot, off, scale = D.member_table(env, hidden)
    k = len(extra)
    return (np.concatenate([slot, 2 + np.arange(k, dtype=np.int32)]), np.concatenate([off, np.zeros(k, np.int64)]),
            np.concatenate([scale, np.zeros(k, np.float32)]))


@pytest.mark.parametrize("case", NULL_CASES, ids=D.case_id)
def test_null_form_after_each_kind_of_evaluation(case):
    from dne_hip import _lib
    env, hidden, nl = case
    kind, dim = SS.kind_id(env), S.N.BC_DIM[env]
    e = G.device_engine(case, 16)
    try:
        rs = np.random.RandomState(5)
        extra = (rs.randn(2, e.P) * 0.3).astype(np.float32)
        th = D.load_members(e, case, extra=extra)                                  # 9 members; base slots 0 and 1
        seeds = D.spread_seeds(case, th, n=9, want=3) if env == "cartpole" else SS.mixed_seeds(9)
        seeds = np.concatenate([seeds, np.array([12345], np.uint32)])              # (five pairs take ten)
        slot, off, scale = e_members(case, extra)
        idx = np.array([100, 7777, 31, 0, 55555], np.int64)
        parent = np.full(9, -1, np.int32); gidx = (np.arange(9, dtype=np.int64) * 1009 + 3)
        evaluations = {
            "eval_members": lambda n, t: e.eval_members(n, t, seeds[:n]),
            "es_eval": lambda n, t: e.es_eval(idx[:(n + 1) // 2], D.SIGMA, t, seeds[:2 * ((n + 1) // 2)]),
            "dense_ga_eval": lambda n, t: e.dense_ga_eval(parent[:n], gidx[:n], np.zeros(n, np.float32), t, seeds[:n]),
        }
        for A in (70, 0):
            arch = rs.uniform(-2, 2, (A, dim)).astype(np.float32)
            load(e, arch)
            for which, run in evaluations.items():
                for n in (1, 3, 5, 9):
                    if A + n - 1 < 1:
                        continue
                    for tslimit in (7, OWN[env]):
                        e.set_members(slot, off, scale)
                        run(n, tslimit)
                        got = e.dense_novelty_pool(10, n=n)                         # k_dense_bc is launched by this call
                        bc = _lib.dense_bc_host(kind, e.dense_final_state(n))
                        assert S.same(got, _lib.dense_novelty_pool_host(bc, arch, 10)), (which, A, n, tslimit)
                        assert same_bits(e.dense_bc(n), bc)
                ran = 10 if which == "es_eval" else 9                                 # (five pairs)
                with pytest.raises(_lib.DneError, match="dne_dense_novelty_pool: %d members asked for, the last evaluation ran %d" % (ran + 1, ran)):
                    e.dense_novelty_pool(2, n=ran + 1)
            assert same_bits(e.dense_archive(), arch)
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- 3. the gather ----------------------------------------------------------------------------------------------------------------------------------------
def roots(n, seed=0):
    return np.full(n, -1, np.int32), (np.arange(n, dtype=np.int64) * 1009 + 3 + 77 * seed), np.zeros(n, np.float32)


@pytest.mark.parametrize("dim", S.DIMS)
def test_gather_appends_members_by_index(handles, dim):
    from dne_hip import _lib
    e = handles[dim]
    e.dense_ga_eval(*roots(9, seed=1), 30, SS.mixed_seeds(9))
    bc = e.dense_bc(9)
    assert same_bits(bc, _lib.dense_bc_host(e.env_kind, e.dense_final_state(9)))
    base = S.cell("random", dim, 3, 9)[1]
    for members in (list(range(9)), list(range(8, -1, -1)), [4, 4, 0, 8, 4], [7], [0], [8]):
        load(e, base)
        e.dense_archive_append_members(members)
        want = np.concatenate([base, bc[members]])
        assert same_bits(e.dense_archive(), want), members
        assert S.same(e.dense_novelty_pool(2), _lib.dense_novelty_pool_host(bc, want, 2))          # a scoring call sees the new points
    e.dense_archive_clear()
    e.dense_archive_append_members([2, 5])                                                         # onto an empty archive
    assert same_bits(e.dense_archive(), bc[[2, 5]])


@pytest.mark.parametrize("dim", S.DIMS)
def test_gather_across_two_reallocations_of_the_archive(dim):
    from dne_hip import _lib
    cap0 = _lib.MAZE_ARCHIVE_CAP0
    e = G.device_engine(LINEAR[dim], 9)                                                            # an archive that has never been allocated
    try:
        e.dense_ga_eval(*roots(9, seed=2), 30, SS.mixed_seeds(9))                                  # the gather's own call forms the BCs
        rs = np.random.RandomState(5)
        want = np.zeros((0, dim), np.float32)
        crossed = set()
        bc = None
        while len(want) <= 2 * cap0 + 9:
            members = rs.randint(0, 9, size=int(rs.randint(1, 10)))
            before = len(want)
            e.dense_archive_append_members(members)
            bc = e.dense_bc(9) if bc is None else bc
            want = np.concatenate([want, bc[members]])
            crossed |= {c for c in (cap0, 2 * cap0) if before <= c < len(want)}
            if before <= cap0 < len(want) or before <= 2 * cap0 < len(want) or before == 0:
                assert same_bits(e.dense_archive(), want), len(want)
                assert S.same(e.dense_novelty_pool(25), _lib.dense_novelty_pool_host(bc, want, 25)), len(want)
        assert crossed == {cap0, 2 * cap0} and same_bits(e.dense_archive(), want) and e.check_redzones() == 0
    finally:
        e.close()


# ---- 4. what the two calls leave alone ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", S.DIMS)
def test_nothing_else_moved(dim):
    from dne_hip import _lib
    case = LINEAR[dim]
    e = G.device_engine(case, 16)
    try:
        P = e.P
        bank_of = lambda: np.stack([e.dense_ga_get_parent(j) for j in range(e.dense_ga_parents())])
        e.dense_ga_build(G.bank_genomes(P, 3))
        bank = bank_of()
        th = D.load_members(e, case)
        bases = D.base_thetas(case[0], case[1])
        seeds = SS.mixed_seeds(9)
        episodes = e.eval_members(7, 30, seeds[:7])
        e.dense_ga_eval(*G.eval_descriptors(P, 3, 9, seed=2), 30, seeds)
        bc = e.dense_bc(9)
        archive = S.cell("random", dim, 65, 9)[1]
        load(e, archive)
        before = e.dense_novelty(25)
        assert S.same(before, _lib.dense_novelty_host(bc, archive, 25))
        pool = e.dense_novelty_pool(25)
        assert S.same(pool, _lib.dense_novelty_pool_host(bc, archive, 25))
        assert S.same(e.dense_novelty(25), before) and same_bits(e.dense_archive(), archive)       # dne_dense_novelty gives what it gave
        e.dense_archive_append_members([1, 3])
        assert S.same(e.dense_novelty(25, bc=bc), _lib.dense_novelty_host(bc, np.concatenate([archive, bc[[1, 3]]]), 25))
        assert same_bits(e.dense_bc(9), bc) and same_bits(bank_of(), bank)
        for slot in (0, 1):
            assert same_bits(e.get_theta(slot), bases[slot])
        again = e.eval_members(7, 30, seeds[:7])                                                   # dne_set_members' members are their own
        assert all(np.array_equal(a, b) for a, b in zip(episodes, again)) and e.check_redzones() == 0
    finally:
        e.close()


# ---- 5. refusals, the archive read back ----------------------------------------------------------------------------------------------------------------------
def raw(e, name, *args):
    assert getattr(e.lib, name)(e.h, *args) != 0, "%s was not refused" % name
    return e.lib.dne_last_error(e.h).decode()


def refusal(fn):
    from dne_hip import _lib
    with pytest.raises(_lib.DneError) as ei:
        fn()
    return str(ei.value)


@pytest.mark.parametrize("dim", S.DIMS)
def test_refusals_leave_the_archive_as_it_was(dim):
    case = LINEAR[dim]
    e = G.device_engine(case, 16)
    fp, ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    try:
        one, two = np.zeros((1, dim), np.float32), np.zeros((2, dim), np.float32)
        # nothing has been evaluated, the archive is empty
        assert refusal(lambda: e.dense_novelty_pool(1, n=1)) == "dne_dense_novelty_pool: 1 members asked for, the last evaluation ran 0"
        assert refusal(lambda: e.dense_archive_append_members([0])) == "dne_dense_archive_append_members: index 0 is member 0, the last evaluation ran 0"
        assert refusal(lambda: e.dense_novelty_pool(1, one)) == "dne_dense_novelty_pool: the pool is empty (one member, no archive point)"
        assert e.dense_archive_size() == 0 and e.dense_novelty_last_ms() == -1.0
        e.dense_ga_eval(*roots(4, seed=3), 20, SS.mixed_seeds(4))                                  # the last evaluation ran 4 members
        assert refusal(lambda: e.dense_novelty_pool(1, n=1)) == "dne_dense_novelty_pool: the pool is empty (one member, no archive point)"
        assert e.dense_archive_size() == 0
        arch = np.random.RandomState(9).uniform(-1, 1, (70, dim)).astype(np.float32)
        e.dense_archive_append(arch)
        members = np.array([0, 3, 4], np.int32)
        for got, want in (
                (refusal(lambda: e.dense_novelty_pool(0, two)), "dne_dense_novelty_pool: k = 0, at least one neighbour is needed"),
                (refusal(lambda: e.dense_novelty_pool(-3, two)), "dne_dense_novelty_pool: k = -3, at least one neighbour is needed"),
                (refusal(lambda: e.dense_novelty_pool(33, two)), "dne_dense_novelty_pool: k = 33, the kernel keeps at most DNE_DENSE_NOVELTY_KMAX = 32 neighbours"),
                (refusal(lambda: e.dense_novelty_pool(1, one[:0])), "dne_dense_novelty_pool: n = 0, at least one point is needed"),
                (refusal(lambda: e.dense_novelty_pool(1, n=0)), "dne_dense_novelty_pool: n = 0, at least one point is needed"),
                (refusal(lambda: e.dense_novelty_pool(1, n=-1)), "dne_dense_novelty_pool: n = -1, at least one point is needed"),
                (refusal(lambda: e.dense_novelty_pool(1, n=5)), "dne_dense_novelty_pool: 5 members asked for, the last evaluation ran 4"),
                (raw(e, "dne_dense_novelty_pool", fp(two), 2, 2, None), "dne_dense_novelty_pool: no output buffer"),
                (raw(e, "dne_dense_novelty_pool", None, 3, 2, None), "dne_dense_novelty_pool: no output buffer"),
                (refusal(lambda: e.dense_archive_append_members([])), "dne_dense_archive_append_members: count = 0, at least one member is needed"),
                (raw(e, "dne_dense_archive_append_members", ip(members), -2), "dne_dense_archive_append_members: count = -2, at least one member is needed"),
                (raw(e, "dne_dense_archive_append_members", None, 2), "dne_dense_archive_append_members: no member indices"),
                (refusal(lambda: e.dense_archive_append_members([0, -1])), "dne_dense_archive_append_members: index 1 is member -1, the last evaluation ran 4"),
                (refusal(lambda: e.dense_archive_append_members(members)), "dne_dense_archive_append_members: index 2 is member 4, the last evaluation ran 4")):
            assert got == want
            assert e.dense_archive_size() == 70 and same_bits(e.dense_archive(), arch), want       # a refused call leaves the archive as it was
        # the maze's pool calls keep refusing kind 8
        for fn, name in ((lambda: e.maze_novelty_pool(2, np.zeros((2, 2), np.float32)), "dne_maze_novelty_pool"),
                         (lambda: e.maze_archive_append_members([0]), "dne_maze_archive_append_members")):
            assert refusal(fn) == "%s needs a DNE_KIND_MAZE engine (this one: kind 8)" % name
        assert e.dense_archive_size() == 70 and same_bits(e.dense_archive(), arch) and e.check_redzones() == 0
    finally:
        e.close()


def test_the_other_episodic_kinds_refuse_the_new_calls():
    from dne_hip import _lib
    fp, dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_double)),
                  lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
    buf, out, members = np.zeros((4, 4), np.float32), np.zeros(4, np.float64), np.zeros(2, np.int32)
    for name in ("MAZE", "CARTPOLE", "PENDULUM", "MJMAZE"):
        kind = getattr(_lib, "KIND_" + name)
        kw = dict(hidden=64, ac_mode="continuous", nonlin="tanh") if kind in _lib.MUJOCO_KINDS else {}
        e = _lib.Engine(kind, 1 if kind == _lib.KIND_PENDULUM else 2, max_members=4, **kw)
        try:
            if kind in (_lib.KIND_MAZE, _lib.KIND_MJMAZE):
                e.maze_archive_append(buf[:, :2])
            for call, args in (("dne_dense_novelty_pool", (fp(buf), 2, 1, dp(out))), ("dne_dense_novelty_pool", (None, 2, 1, dp(out))),
                               ("dne_dense_archive_append_members", (ip(members), 2))):
                assert raw(e, call, *args) == "%s needs a DNE_KIND_DENSE engine (this one: kind %d)" % (call, kind)
            assert e.dense_novelty_last_ms() == -1.0
            if kind in (_lib.KIND_MAZE, _lib.KIND_MJMAZE):
                assert e.maze_archive_size() == 4 and same_bits(e.maze_archive(), buf[:, :2])
        finally:
            e.close()


# ---- 6. the driver --------------------------------------------------------------------------------------------------------------------------------------------
DRIVER_CASES = {"maze-linear": ("maze", (), "relu"), "cartpole-linear": ("cartpole", (), "relu"), "cartpole-5-33": ("cartpole", (5, 33), "relu")}
GAME = {"maze": "maze", "cartpole": "gym.CartPole-v1"}


def _same_run(a, b):
    (ta, va, sa), (tb, vb, sb) = a, b
    ok = (ta, va) == (tb, vb) and sa.it == sb.it and [o.seeds for o in sa.population] == [o.seeds for o in sb.population]
    ok = ok and [o.rewards for o in sa.population] == [o.rewards for o in sb.population] and sa.elite.seeds == sb.elite.seeds
    ok = ok and [o.novelty for o in sa.population] == [o.novelty for o in sb.population] and same_bits(sa.archive, sb.archive)
    ok = ok and (sa.game, sa.model, sa.num_params, sa.algo, sa.k, sa.archive_prob) == (sb.game, sb.model, sb.num_params, sb.algo, sb.k, sb.archive_prob)
    return ok and (sa.curr_solution, sa.timesteps_so_far, sa.num_frames) == (sb.curr_solution, sb.timesteps_so_far, sb.num_frames) and S.same_stream(sa.stream, sb.stream)


@pytest.mark.parametrize("name", sorted(DRIVER_CASES))
def test_driver_on_the_device_equals_the_host_engine(oracle, tmp_path, name):
    """dense_ns_main on a live handle -- one it opens itself where the routing has the shape -- against the same driver on DenseGaNsHostEngine,
    row by row: two generations, then two more resumed, on each side"""
    from dne_hip import ga_gpu
    case = DRIVER_CASES[name]
    exp = S.exp(GAME[case[0]], model=None if case[1] else "LinearClassifier", ns={"k": 3, "archive_prob": 0.5})
    own = not case[1]                                                                              # LinearClassifier: the driver builds the engine
    hip = None if own else G.device_engine(case, 10)
    host = S.host_engine(case, 10)
    try:
        for it in (2, 4):
            a = ga_gpu.dense_ns_main(str(tmp_path / "hip"), engine=hip, noise=S.shared_noise(), seed=4, max_iters=2, **exp)
            b = ga_gpu.dense_ns_main(str(tmp_path / "host"), engine=host, noise=S.shared_noise(), seed=4, max_iters=2, **exp)
            assert a[2].it == it and a[2].algo == "ga_ns" and _same_run(a, b)
            assert D.same_rows(S.log_rows(tmp_path / "hip"), S.log_rows(tmp_path / "host"))
            if hip is not None:
                assert same_bits(hip.dense_archive(), host.dense_archive()) and hip.dense_ga_parents() == host.dense_ga_parents()
                assert all(same_bits(hip.dense_ga_get_parent(j), host.bank[j]) for j in range(hip.dense_ga_parents()))
        assert len(a[2].archive) > 0 and len(S.log_rows(tmp_path / "hip")) == 4
        if hip is not None:
            assert hip.check_redzones() == 0
    finally:
        if hip is not None:
            hip.close()


def test_a_16_16_dense_handle_on_the_maze_is_the_kind_maze_run(oracle, tmp_path):
    from dne_hip import _lib, ga_gpu
    exp = S.exp("maze", model="SimpleClassifier", episode_cutoff_mode=400, ns={"k": 3, "archive_prob": 0.5})
    mz = _lib.Engine(_lib.KIND_MAZE, 2, max_members=10)
    dn = _lib.Engine(_lib.KIND_DENSE, 2, max_members=10, env=_lib.KIND_MAZE, hidden=(16, 16), nonlin="relu")
    try:
        _, _, ref = ga_gpu.main(str(tmp_path / "maze"), engine=mz, noise=S.shared_noise(), seed=4, max_iters=3, **exp)
        _, _, got = ga_gpu.dense_ns_main(str(tmp_path / "dense"), engine=dn, noise=S.shared_noise(), seed=4, max_iters=3, **{k: v for k, v in exp.items() if k != "model"})
        assert D.same_rows(S.log_rows(tmp_path / "dense"), S.log_rows(tmp_path / "maze")) and len(S.log_rows(tmp_path / "dense")) == 3
        assert [o.seeds for o in got.population] == [o.seeds for o in ref.population] and [o.novelty for o in got.population] == [o.novelty for o in ref.population]
        assert len(got.archive) > 0 and same_bits(got.archive, ref.archive) and same_bits(dn.dense_archive(), mz.maze_archive())
        assert all(same_bits(dn.dense_ga_get_parent(j), mz.maze_ga_get_parent(j)) for j in range(3)) and S.same_stream(got.stream, ref.stream)
        assert dn.check_redzones() == 0
    finally:
        mz.close(); dn.close()
