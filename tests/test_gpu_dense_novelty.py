"""GPU: novelty over final states on the dense kind (csrc/dense_novelty.h on a DNE_KIND_DENSE engine), BIT FOR BIT: k_dense_novelty<2> and <4>
against the CPU twin on the CPU file's whole grid (k = 40 is a refusal here) and, for D = 2, against k_maze_novelty of a DNE_KIND_MAZE handle;
k_dense_bc and the NULL forms behind every kind of evaluation; the archive across its first allocation and two doublings; every refusal with
the archive read back; and nses_gpu.main on live handles against DenseNoveltyHostEngine and against the SimpleClassifier run."""
import ctypes as C

import numpy as np
import pytest

import dense_ga_support as G
import dense_novelty_support as S
import dense_support as D
import maze_support as MS
import stepenv_support as SS

pytestmark = pytest.mark.gpu

LINEAR = {2: ("maze", (), "relu"), 4: ("cartpole", (), "relu")}
NULL_CASES = (("maze", (), "relu"), ("cartpole", (5, 33), "relu"), ("pendulum", (64,), "tanh"))
OWN = {"maze": 400, "cartpole": 500, "pendulum": 200}
DEVICE_KS = tuple(k for k in S.KS if k <= S.KMAX)


@pytest.fixture(scope="module")
def handles():
    """one live handle per D (no hidden layer, 16 members) for the calls that take their points from the host"""
    es = {dim: D.device_engine(case, 16) for dim, case in LINEAR.items()}
    yield es
    for e in es.values():
        assert e.check_redzones() == 0
        e.close()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(SS.bits(a), SS.bits(b))


# ---- 1. the kernel against the twin, and against k_maze_novelty ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", S.DIMS)
@pytest.mark.parametrize("name", S.SETS)
def test_kernel_equals_the_twin_on_every_shape(handles, name, dim):
    from dne_hip import _lib
    e = handles[dim]
    assert e.dense_bc_dim() == dim
    for narch in S.SIZES:
        mem, arch = S.point_set(name, dim, narch)
        e.dense_archive_clear()
        e.dense_archive_append(arch)
        assert e.dense_archive_size() == narch
        for k in DEVICE_KS:
            want = _lib.dense_novelty_host(mem, arch, k)
            assert S.same(want, S.contract_of(name, dim, narch, k))
            for n in S.COUNTS:
                got = e.dense_novelty(k, mem[:n])
                assert got.dtype == np.float64 and S.same(got, want[:n]), (name, dim, narch, n, k, got, want[:n])
        assert e.dense_novelty_last_ms() > 0
        with pytest.raises(_lib.DneError, match="k = 40, the kernel keeps at most DNE_DENSE_NOVELTY_KMAX = 32"):
            e.dense_novelty(40, mem)
        assert same_bits(e.dense_archive(), arch)


def test_two_coordinates_equal_k_maze_novelty(handles):
    from dne_hip import _lib
    e = handles[2]
    mz = _lib.Engine(_lib.KIND_MAZE, 2, max_members=16)
    try:
        for name in S.SETS:
            for narch in (1, 63, 65, 1025, 2049):
                mem, arch = S.point_set(name, 2, narch)
                e.dense_archive_clear(); e.dense_archive_append(arch)
                mz.maze_archive_clear(); mz.maze_archive_append(arch)
                for k in DEVICE_KS:
                    assert S.same(e.dense_novelty(k, mem), mz.maze_novelty(k, mem)), (name, narch, k)
    finally:
        mz.close()


# ---- 2. the NULL forms behind every kind of evaluation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NULL_CASES, ids=D.case_id)
def test_null_forms_after_each_kind_of_evaluation(case):
    from dne_hip import _lib
    env, hidden, nl = case
    kind, dim = SS.kind_id(env), S.BC_DIM[env]
    e = G.device_engine(case, 16)
    try:
        assert e.dense_bc_dim() == dim
        rs = np.random.RandomState(5)
        extra = (rs.randn(2, e.P) * 0.3).astype(np.float32)
        th = D.load_members(e, case, extra=extra)                                  # 9 members; base slots 0 and 1
        seeds = D.spread_seeds(case, th, n=9, want=3) if env == "cartpole" else SS.mixed_seeds(9)
        seeds = np.concatenate([seeds, np.array([12345], np.uint32)])              # (five pairs take ten)
        arch = rs.uniform(-2, 2, (70, dim)).astype(np.float32)
        e.dense_archive_append(arch)
        slot, off, scale = (np.array(a) for a in e_members(case, extra))
        idx = np.array([100, 7777, 31, 0, 55555], np.int64)
        parent = np.full(9, -1, np.int32); gidx = (np.arange(9, dtype=np.int64) * 1009 + 3)
        evaluations = {
            "eval_members": lambda n, t: e.eval_members(n, t, seeds[:n])[2],
            "es_eval": lambda n, t: e.es_eval(idx[:(n + 1) // 2], D.SIGMA, t, seeds[:2 * ((n + 1) // 2)])[2].reshape(-1)[:n],
            "dense_ga_eval": lambda n, t: e.dense_ga_eval(parent[:n], gidx[:n], np.zeros(n, np.float32), t, seeds[:n])[2],
        }
        seen = []
        for which, run in evaluations.items():
            for n in (1, 3, 5, 9):
                for tslimit in (1, 7, OWN[env]):
                    e.set_members(slot, off, scale)
                    ln = run(n, tslimit)
                    rec = e.dense_final_state(n)
                    bc = e.dense_bc(n)
                    assert bc.dtype == np.float32 and same_bits(bc, _lib.dense_bc_host(kind, rec)), (which, n, tslimit)
                    assert same_bits(bc, e.dense_bc(n))                             # formed once: the second call reads the same buffer
                    got = e.dense_novelty(10, n=n)
                    assert S.same(got, _lib.dense_novelty_host(bc, arch, 10)), (which, n, tslimit)
                    if tslimit == 7:
                        assert not same_bits(bc, seen[-1])                          # a second evaluation replaces the BCs (one step, then seven)
                    seen.append(bc)
                    if env == "cartpole" and which == "eval_members" and n == 9 and tslimit == OWN[env]:
                        assert len(set(np.asarray(ln).tolist())) >= 3
            ran = 10 if which == "es_eval" else 9                                     # (five pairs)
            with pytest.raises(_lib.DneError, match="dne_dense_bc: %d members asked for, the last evaluation ran %d" % (ran + 1, ran)):
                e.dense_bc(ran + 1)
        assert same_bits(e.dense_archive(), arch) and e.check_redzones() == 0
    finally:
        e.close()


def e_members(case, extra):
    """load_members' descriptors once more (it returns the thetas only)"""
    env, hidden, _ = case
    slot, off, scale = D.member_table(env, hidden)
    k = len(extra)
    return (np.concatenate([slot, 2 + np.arange(k, dtype=np.int32)]), np.concatenate([off, np.zeros(k, np.int64)]),
            np.concatenate([scale, np.zeros(k, np.float32)]))


# ---- 3. the archive ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", S.DIMS)
def test_archive_across_its_first_allocation_and_two_doublings(dim):
    from dne_hip import _lib
    case = LINEAR[dim]
    env, hidden, nl = case
    e = D.device_engine(case, 16)
    try:
        th = D.load_members(e, case)
        seeds = SS.mixed_seeds(7)
        rs = np.random.RandomState(dim)
        mirror = np.zeros((0, dim), np.float32)
        assert e.dense_archive_size() == 0 and e.dense_archive().shape == (0, dim)
        for rnd in range(2):
            tslimit = 5
            for count, null in ((1, True), (62, False), (1, True), (1, False), (64, False), (1000, False)):   # 64 is the first allocation; 65, 129 and 1129 outgrow it
                if null:
                    tslimit += 3
                    e.eval_members(7, tslimit, seeds)
                    pts = e.dense_bc(count)
                    e.dense_archive_append(n=count)
                    nov = e.dense_novelty(2, n=7)                                  # between the append and the next evaluation: stream order
                    e.eval_members(7, 1, seeds)                                    # ... which must not reach the appended point: one step, other BCs
                    assert not same_bits(e.dense_bc(count), pts)
                else:
                    pts = rs.uniform(-3, 3, (count, dim)).astype(np.float32)
                    e.dense_archive_append(pts)
                mirror = np.concatenate([mirror, pts])
                assert e.dense_archive_size() == len(mirror) and same_bits(e.dense_archive(), mirror), (rnd, count, null)
                if null:
                    e.eval_members(7, tslimit, seeds)
                    assert S.same(nov, _lib.dense_novelty_host(e.dense_bc(7), mirror, 2))
            assert len(mirror) == 1129
            assert S.same(e.dense_novelty(32, mirror[:9]), _lib.dense_novelty_host(mirror[:9], mirror, 32))
            e.dense_archive_clear()
            mirror = np.zeros((0, dim), np.float32)
            assert e.dense_archive_size() == 0
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- 4. what is refused, the archive left as it was ------------------------------------------------------------------------------------------------------------------
def raw(e, name, *args):
    assert getattr(e.lib, name)(e.h, *args) != 0, "%s was not refused" % name
    return e.lib.dne_last_error(e.h).decode()


def refusal(fn):
    from dne_hip import _lib
    with pytest.raises(_lib.DneError) as ei:
        fn()
    return str(ei.value)


@pytest.mark.parametrize("dim", S.DIMS)
def test_refusals_leave_the_archive_alone(dim):
    case = LINEAR[dim]
    e = D.device_engine(case, 16)
    fp, dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    try:
        one = np.zeros((1, dim), np.float32); out = np.zeros(16, np.float64)
        assert refusal(lambda: e.dense_novelty(1, one)) == "dne_dense_novelty: the archive is empty (dne_dense_archive_append)"
        assert refusal(lambda: e.dense_archive_append(n=1)) == "dne_dense_archive_append: 1 members asked for, the last evaluation ran 0"
        assert refusal(lambda: e.dense_bc(1)) == "dne_dense_bc: 1 members asked for, the last evaluation ran 0"
        assert e.dense_novelty_last_ms() == -1.0
        arch = np.random.RandomState(9).uniform(-1, 1, (70, dim)).astype(np.float32)
        e.dense_archive_append(arch)
        D.load_members(e, case)
        e.eval_members(3, 4, SS.mixed_seeds(3))
        for got, want in (
                (refusal(lambda: e.dense_archive_append(one[:0])), "dne_dense_archive_append: n = 0, at least one point is needed"),
                (refusal(lambda: e.dense_archive_append(n=0)), "dne_dense_archive_append: n = 0, at least one point is needed"),
                (refusal(lambda: e.dense_archive_append(n=4)), "dne_dense_archive_append: 4 members asked for, the last evaluation ran 3"),
                (refusal(lambda: e.dense_novelty(2, one[:0])), "dne_dense_novelty: n = 0, at least one point is needed"),
                (refusal(lambda: e.dense_novelty(2, n=-1)), "dne_dense_novelty: n = -1, at least one point is needed"),
                (refusal(lambda: e.dense_novelty(2, n=4)), "dne_dense_novelty: 4 members asked for, the last evaluation ran 3"),
                (refusal(lambda: e.dense_novelty(0, one)), "dne_dense_novelty: k = 0, at least one neighbour is needed"),
                (refusal(lambda: e.dense_novelty(33, one)), "dne_dense_novelty: k = 33, the kernel keeps at most DNE_DENSE_NOVELTY_KMAX = 32 neighbours"),
                (raw(e, "dne_dense_novelty", fp(one), 1, 2, None), "dne_dense_novelty: no output buffer"),
                (raw(e, "dne_dense_novelty", None, 3, 2, None), "dne_dense_novelty: no output buffer"),
                (raw(e, "dne_dense_archive_get", fp(np.zeros((69, dim), np.float32)), 69), "dne_dense_archive_get: room for 69 points, the archive holds 70"),
                (raw(e, "dne_dense_archive_get", None, 70), "dne_dense_archive_get: no buffer"),
                (refusal(lambda: e.dense_bc(0)), "dne_dense_bc: 0 members asked for, the last evaluation ran 3"),
                (refusal(lambda: e.dense_bc(4)), "dne_dense_bc: 4 members asked for, the last evaluation ran 3"),
                (raw(e, "dne_dense_bc", 3, None), "dne_dense_bc: no output buffer")):
            assert got == want
            assert e.dense_archive_size() == 70 and same_bits(e.dense_archive(), arch)
        # the maze's calls keep refusing kind 8
        for fn, name in ((lambda: e.maze_archive_append(np.zeros((1, 2), np.float32)), "dne_maze_archive_append"), (lambda: e.maze_archive_clear(), "dne_maze_archive_clear"),
                         (lambda: e.maze_archive_size(), "dne_maze_archive_size"), (lambda: e.maze_archive(), "dne_maze_archive_size"),
                         (lambda: e.maze_novelty(2, np.zeros((1, 2), np.float32)), "dne_maze_novelty"),
                         (lambda: e.maze_novelty_pool(2, np.zeros((2, 2), np.float32)), "dne_maze_novelty_pool"),
                         (lambda: e.maze_archive_append_members([0]), "dne_maze_archive_append_members"), (lambda: e.maze_final_state(1), "dne_maze_final_state")):
            assert refusal(fn) == "%s needs a DNE_KIND_MAZE engine (this one: kind 8)" % name
        assert e.dense_archive_size() == 70 and same_bits(e.dense_archive(), arch) and e.check_redzones() == 0
    finally:
        e.close()


def test_the_other_episodic_kinds_refuse_the_dense_calls():
    from dne_hip import _lib
    fp, dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    buf, out = np.zeros((4, 4), np.float32), np.zeros(4, np.float64)
    for name in ("MAZE", "CARTPOLE", "PENDULUM", "MJMAZE"):
        kind = getattr(_lib, "KIND_" + name)
        kw = dict(hidden=64, ac_mode="continuous", nonlin="tanh") if kind in _lib.MUJOCO_KINDS else {}
        e = _lib.Engine(kind, 1 if kind == _lib.KIND_PENDULUM else 2, max_members=4, **kw)
        try:
            for call, args in (("dne_dense_bc_dim", ()), ("dne_dense_bc", (1, fp(buf))), ("dne_dense_archive_append", (fp(buf), 1)), ("dne_dense_archive_clear", ()),
                               ("dne_dense_archive_size", ()), ("dne_dense_archive_get", (fp(buf), 4)), ("dne_dense_novelty", (fp(buf), 1, 1, dp(out)))):
                assert raw(e, call, *args) == "%s needs a DNE_KIND_DENSE engine (this one: kind %d)" % (call, kind)
            assert e.dense_novelty_last_ms() == -1.0
            if kind in (_lib.KIND_MAZE, _lib.KIND_MJMAZE):
                assert e.maze_archive_size() == 0
        finally:
            e.close()


# ---- 5. the driver -----------------------------------------------------------------------------------------------------------------------------------------------------
DRIVER_CASES = (
    ("maze", dict(ns={"selection_method": "novelty_prob"})),
    ("cartpole", dict(algo_type="nsr", return_proc_mode="centered_rank")),
    ("cartpole", dict(return_proc_mode="sign", ns={"num_rollouts": 3, "selection_method": "novelty_prob"})),
)


@pytest.mark.parametrize("env,over", DRIVER_CASES, ids=("maze-prob", "cartpole-nsr", "cartpole-mean-bc"))
def test_driver_on_its_own_engine_equals_the_host_engine(tmp_path, env, over):
    import copy
    from dne_hip import nses_gpu
    live = lambda sub, iters: nses_gpu.main(str(tmp_path / sub), engine=None, noise=D.shared_noise(), seed=4, max_iters=iters, **S.exp(env, **copy.deepcopy(over)))
    want, _ = S.run(tmp_path / "host", 3, env, **copy.deepcopy(over))
    got = live("live", 3)
    assert S.same_state(got, want) and D.same_rows(D.log_rows(tmp_path / "live"), D.log_rows(tmp_path / "host"))
    assert (got.game, got.model, got.num_params) == (S.GAMES[env], "LinearClassifier", want.num_params)
    live("resumed", 1)
    assert S.same_state(live("resumed", 2), want)


def test_a_16_16_dense_handle_on_the_maze_is_the_kind_maze_run(tmp_path):
    from dne_hip import _lib, nses_gpu
    over = dict(algo_type="nsr", ns={"selection_method": "novelty_prob"})
    mz = _lib.Engine(_lib.KIND_MAZE, 2, max_members=8)
    dn = _lib.Engine(_lib.KIND_DENSE, 2, max_members=8, env=_lib.KIND_MAZE, hidden=(16, 16), nonlin="relu")
    try:
        ref = nses_gpu.main(str(tmp_path / "maze"), engine=mz, noise=D.shared_noise(), seed=4, max_iters=3, **S.exp("maze", model="SimpleClassifier", **dict(over)))
        got = nses_gpu.main(str(tmp_path / "dense"), engine=dn, noise=D.shared_noise(), seed=4, max_iters=3, **S.exp("maze", model=None, **dict(over)))
        assert S.same_state(got, ref) and D.same_rows(D.log_rows(tmp_path / "dense"), D.log_rows(tmp_path / "maze"))
        assert same_bits(dn.dense_archive(), mz.maze_archive()) and dn.check_redzones() == 0
    finally:
        mz.close(); dn.close()
