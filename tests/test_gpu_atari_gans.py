"""GPU: GA-NS on Atari (csrc/ram_novelty.h), BIT FOR BIT: k_ram_novelty_pool against the CPU twin, novelty and
neighbours, on the grid (the kernel's own tile size +-1 on both sides of the seam included) and the edge inputs; the NULL form behind real
evaluations of a KIND_GA, a KIND_GA_LARGE and a bc_final_only ES engine; the n = 1 pool against dne_novelty_knn; k_ram_archive_gather in order,
reversed, repeated and across two reallocations; what the new calls leave alone; every refusal with the archive read back; and
ga_gpu.atari_ns_main on a live handle against the same driver on AtariGaNsHostEngine."""
import ctypes as C

import numpy as np
import pytest

import atari_gans_support as S
import ga_store_support as G
import step_tap_support as T

pytestmark = pytest.mark.gpu
NACT = 18


@pytest.fixture(scope="module")
def handle():
    """one KIND_GA handle with record_bc for the calls that take their points from the host"""
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_GA, NACT, max_members=16, record_bc=True)
    yield e
    assert e.check_redzones() == 0
    e.close()


def load(e, archive):
    """bring the resident archive to `archive`, appending only what is new when it continues what is there"""
    have = e.archive_size()
    if have > len(archive) or (have and not np.array_equal(e.archive_get_points(0, have), archive[:have])):
        e.archive_clear()
        have = 0
    if len(archive) > have:
        e.archive_append_points(archive[have:])
    assert e.archive_size() == len(archive)


def pool(e, k, bc=None, n=None):
    return e.ram_novelty_pool(k, bc=bc, n=n, neighbours=True)


def twin(bc, archive, k):
    from dne_hip import _lib
    return _lib.ram_novelty_pool_host(bc, archive, k, neighbours=True)


def assert_same(got, want, tag):
    assert got[1].dtype == np.int32 and got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), tag
    assert got[0].dtype == np.float64 and got[0].shape == want[0].shape and S.same(got[0], want[0]), tag


# ---- 1. the kernel against the twin ------------------------------------------------------------------------------------------------------------------
def test_shapes_are_the_ones_asked_for():
    assert set((0, 1, 31, 32, 33, 1023, 1024, 1025)) <= set(S.GPU_ARCHIVES) and S.GPU_COUNTS == (1, 9, 33, 65) and S.GPU_KS == (1, 25, 32)
    assert set((S.TILE - 1, S.TILE, S.TILE + 1)) <= set(S.GPU_ARCHIVES)                                # the archive ends at a tile's edge -1, 0, +1
    assert all(any(A + n == S.TILE + d for A in S.GPU_ARCHIVES) for n in (9, 33) for d in (-1, 0, 1))   # ... and the population does
    assert S.MEMBERS == 4 and all(n % S.MEMBERS for n in (1, 9, 33, 65))                                # every n leaves a partial last member tile


@pytest.mark.parametrize("name", S.SETS)
def test_kernel_equals_the_twin_on_every_shape(handle, name):
    e = handle
    mem, arch = S.point_set(name)
    for A in sorted(S.GPU_ARCHIVES):
        load(e, arch[:A])
        for n in S.GPU_COUNTS:
            if A + n - 1 < 1:
                continue
            for k in S.GPU_KS:
                assert_same(pool(e, k, mem[:n]), twin(mem[:n], arch[:A], k), (name, A, n, k))
        assert e.ram_novelty_last_ms() > 0 and (A == 0 or np.array_equal(e.archive_get_points(0, A), arch[:A]))


def test_kernel_equals_the_twin_on_the_edge_inputs(handle):
    e = handle
    for name, (bc, archive, ks) in sorted(S.edge_cases().items()):
        load(e, archive)
        for k in ks:
            for n in range(1, len(bc) + 1):
                if len(archive) + n - 1 >= 1:
                    assert_same(pool(e, k, bc[:n]), twin(bc[:n], archive, k), (name, k, n))
    bc, archive, _ = S.edge_cases()["extremes"]
    load(e, archive[:1])
    assert pool(e, 1, bc[:1])[0][0] == np.sqrt(np.sqrt(float(S.S_MAX)) ** 2 + 0.0)                      # the largest S there is


# ---- 2. the NULL form behind real evaluations ------------------------------------------------------------------------------------------------------------
def _genomes(kind):
    """9 genomes: three roots and six children whose parents alternate, so that an engine that groups members by parent reorders them"""
    hi = G.last_offset(kind)
    roots = [(17, ), (hi, ), (1_000_003, )]
    return [roots[0], roots[1] + ((5, 0.002), ), roots[2] + ((7, 0.004), ), roots[1], roots[0] + ((9, 0.002), ), roots[2] + ((11, -0.002), ),
            roots[1] + ((13, 0.001), ), roots[2], roots[0] + ((15, 0.004), )]


@pytest.mark.parametrize("kind", (T.KIND_GA, T.KIND_GA_LARGE), ids=("ga", "ga_large"))
def test_null_form_after_ga_eval_powers(kind):
    from dne_hip import _lib
    e = _lib.Engine(kind, NACT, max_members=16, record_bc=True)
    try:
        e.noise_upload(G.noise_of(kind))
        e.ga_set_init_scale(G.scale_by(kind))
        with pytest.raises(_lib.DneError, match="no evaluation has left final RAM states yet"):
            e.ram_novelty_pool(1, n=2)
        genomes = _genomes(kind)
        _, _, _, bc = e.ga_eval_powers(genomes, 20, T.tap_seeds(9), want_bc=True)
        who = e.debug_members()[3]
        arch = S.point_set("random")[1]
        for A in (0, 3, S.TILE + 1):
            load(e, arch[:A])
            for k in (1, 3, 25):
                assert_same(pool(e, k), twin(bc, arch[:A], k), (kind, A, k))                           # all 9, in the caller's order
                assert_same(pool(e, k, n=5), twin(bc[:5], arch[:A], k), (kind, A, k, 5))               # the first 5 are the population
        with pytest.raises(_lib.DneError, match="10 members asked for, the last evaluation ran 9"):
            e.ram_novelty_pool(1, n=10)
        # the gather takes the caller's indices whatever order the engine ran its members in
        load(e, arch[:2])
        e.archive_append_members([8, 0, 4, 4])
        assert np.array_equal(e.archive_get_points(0, 6), np.concatenate([arch[:2], bc[[8, 0, 4, 4]]]))
        assert sorted(who.tolist()) == list(range(9))
        if G.knobs_of(kind)[1]:                                                                        # DNE_GA_SORT: the rows of bc are NOT in the caller's order
            assert who.tolist() != list(range(9))
        # the same member table evaluated again by eval_members: its caller's order is the engine's row order
        _, _, _, rows = e.eval_members(9, 20, T.tap_seeds(9), want_bc=True)
        load(e, arch[:3])
        assert_same(pool(e, 3), twin(rows, arch[:3], 3), (kind, "eval_members after ga_eval_powers"))
        e.archive_append_members([2, 7])
        assert np.array_equal(e.archive_get_points(3, 2), rows[[2, 7]])
        assert e.check_redzones() == 0
    finally:
        e.close()


def test_null_form_after_es_eval_and_eval_members(oracle, small_noise):
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_ES, NACT, max_members=16, ref_count=16, record_bc=True, bc_final_only=True)
    try:
        e.noise_upload(small_noise)
        e.set_ref_batch(oracle.get_ref_batch(seed=0, batch_size=16, nact=NACT))
        e.set_theta(oracle.es_init_theta(oracle.layout(0, NACT), 0))
        idx = np.array([0, 1_000_000, 4, 2_000_000], np.int64)
        _, _, _, bc = e.es_eval(idx, 0.02, 20, T.tap_seeds(8), want_bc=True)
        arch = S.point_set("random")[1]
        for A in (0, 33):
            load(e, arch[:A])
            assert_same(pool(e, 3), twin(bc, arch[:A], 3), ("es", A))
        e.archive_append_members([7, 0])
        assert np.array_equal(e.archive_get_points(33, 2), bc[[7, 0]])
        e.set_members(np.zeros(6, np.int32), idx[[0, 1, 2, 3, 0, 1]], np.array([0.02, -0.02, 0.0, 0.01, 0.03, 0.01], np.float32))
        _, _, _, bc6 = e.eval_members(6, 20, T.tap_seeds(6), want_bc=True)
        load(e, arch[:4])
        assert_same(pool(e, 2), twin(bc6, arch[:4], 2), "eval_members")
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- 3. the second witness ------------------------------------------------------------------------------------------------------------------------------
def test_one_member_pool_is_novelty_knn(handle):
    e = handle
    for name in S.SETS:
        mem, arch = S.point_set(name)
        for A in (1, 33, S.TILE + 1):
            load(e, arch[:A])
            for m in (0, 1, 7):
                for k in (1, 25, 32):
                    a = e.ram_novelty_pool(k, mem[m:m + 1])
                    b = e.novelty_knn(None, k, bcs=[mem[m:m + 1]])
                    assert S.same(a, b), (name, A, m, k)


# ---- 4. the gather ----------------------------------------------------------------------------------------------------------------------------------------
def test_gather_orders_repeats_and_reallocations():
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_GA, NACT, max_members=16, record_bc=True)
    try:
        e.noise_upload(G.noise_of(T.KIND_GA))
        e.ga_set_init_scale(G.scale_by(T.KIND_GA))
        _, _, _, bc = e.ga_eval_powers(_genomes(T.KIND_GA), 20, T.tap_seeds(9), want_bc=True)
        want = np.zeros((0, S.RAM), np.uint8)
        for members in (list(range(9)), list(range(8, -1, -1)), [3, 3, 3, 0, 8, 0], [5]):
            e.archive_append_members(members)
            want = np.concatenate([want, bc[members]])
            assert e.archive_size() == len(want) and np.array_equal(e.archive_get_points(0, len(want)), want), members
        # two reallocations of the rows (1 MiB = 8192 rows at first, doubling) and of the entry tables (256 at first)
        many = np.resize(np.arange(9), 8192 - len(want) + 3)
        e.archive_append_members(many)
        want = np.concatenate([want, bc[many]])
        more = np.resize(np.arange(8, -1, -1), 8195 * 2 - len(want) + 5)
        e.archive_append_members(more)
        want = np.concatenate([want, bc[more]])
        assert e.archive_size() == len(want) and np.array_equal(e.archive_get_points(0, len(want)), want)
        assert np.array_equal(e.archive_get_points(8190, 7), want[8190:8197])
        # seen by a following pool call and by novelty_knn
        mem = S.point_set("random")[0]
        assert_same(pool(e, 25, mem[:5]), twin(mem[:5], want, 25), "after the gathers")
        assert S.same(e.novelty_knn(None, 7, bcs=[mem[0:1]]), twin(mem[0:1], want, 7)[0])
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- 5. what the new calls leave alone ---------------------------------------------------------------------------------------------------------------------
def test_pool_calls_leave_the_other_state_alone(oracle, small_noise):
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_ES, NACT, max_members=16, ref_count=16, record_bc=True, bc_max_steps=30)
    try:
        e.noise_upload(small_noise)
        e.set_ref_batch(oracle.get_ref_batch(seed=0, batch_size=16, nact=NACT))
        th = oracle.es_init_theta(oracle.layout(0, NACT), 0)
        e.set_theta(th)
        idx = np.array([0, 1_000_000, 4], np.int64)
        _, _, ln = e.es_eval(idx, 0.02, 20, T.tap_seeds(6))
        mem, arch = S.point_set("random")
        entries = [arch[a:a + 1] for a in range(40)]                                                    # one-row entries: a RAM archive both calls read
        rs = np.random.RandomState(3)
        trajs = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in (1, 9, 30)]
        knn, batch = e.novelty_knn(entries, 5, bcs=trajs), e.novelty_batch(entries, ln.reshape(-1), 5)
        members = [a.copy() for a in e.debug_members()]
        got = pool(e, 25, mem[:9])                                                                      # the host form works on any Atari engine
        assert_same(got, twin(mem[:9], arch[:40], 25), "host form on an ES engine")
        assert np.array_equal(e.novelty_knn(entries, 5, bcs=trajs), knn) and np.array_equal(e.novelty_batch(entries, ln.reshape(-1), 5), batch)
        assert np.array_equal(e.get_theta(), th) and all(np.array_equal(a, b) for a, b in zip(members, e.debug_members()))
        assert e.archive_size() == 40 and np.array_equal(e.archive_get_points(0, 40), arch[:40]) and e.check_redzones() == 0
    finally:
        e.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(handle, oracle, small_noise):
    from dne_hip import _lib
    e = handle
    mem, arch = S.point_set("random")
    load(e, arch[:5])

    def check(text, call, *a, **kw):
        with pytest.raises(_lib.DneError, match=text):
            call(*a, **kw)
        assert e.archive_size() == 5 and np.array_equal(e.archive_get_points(0, 5), arch[:5])

    check(r"k = 0, at least one neighbour", e.ram_novelty_pool, 0, mem[:3])
    check(r"k = 33, the kernel keeps at most DNE_RAM_NOVELTY_KMAX = 32", e.ram_novelty_pool, 33, mem[:3])
    check(r"n = 0, at least one member", e.ram_novelty_pool, 1, mem[:0])
    check(r"count = 0, at least one member", e.archive_append_members, [])
    check(r"count = 0, at least one entry", e.archive_get_points, 0, 0)
    check(r"entries 3 .. 5 asked for, the archive holds 5", e.archive_get_points, 3, 3)
    check(r"entries -1 .. 0 asked for", e.archive_get_points, -1, 2)
    out = np.zeros(4)
    p = mem.ctypes.data_as(C.POINTER(C.c_uint8))
    assert e.lib.dne_ram_novelty_pool(e.h, p, 2 ** 31 - 1, 1, out.ctypes.data_as(C.POINTER(C.c_double)), None) != 0     # refused before anything is read
    assert b"would not fit the kernel's 31-bit slot field" in e.lib.dne_last_error(e.h)
    assert e.lib.dne_ram_novelty_pool(e.h, p, 2, 1, None, None) != 0 and b"no output buffer" in e.lib.dne_last_error(e.h)
    assert e.archive_size() == 5 and np.array_equal(e.archive_get_points(0, 5), arch[:5])
    # the empty pool; an archive entry of another length; an archive of another width
    e.archive_clear()
    with pytest.raises(_lib.DneError, match=r"the pool is empty \(one member, no archive point\)"):
        e.ram_novelty_pool(1, mem[:1])
    fresh = _lib.Engine(_lib.KIND_GA, NACT, max_members=16, record_bc=True)
    try:
        for call, args in ((fresh.ram_novelty_pool, (1, None, 2)), (fresh.archive_append_members, ([0], ))):
            with pytest.raises(_lib.DneError, match="no evaluation has left final RAM states yet"):
                call(*args)
        assert fresh.archive_size() == 0
    finally:
        fresh.close()
    load(e, arch[:2])
    two = np.ascontiguousarray(arch[10:12])
    assert e.lib.dne_archive_append(e.h, two.ctypes.data_as(C.POINTER(C.c_uint8)), 2, 128) == 0
    with pytest.raises(_lib.DneError, match=r"archive entry 2 has length 2, a RAM point is an entry of length 1"):
        e.ram_novelty_pool(1, mem[:3])
    with pytest.raises(_lib.DneError, match=r"archive entry 2 has length 2"):
        e.archive_get_points(1, 2)
    assert e.archive_size() == 3 and np.array_equal(e.archive_get_points(0, 2), arch[:2])
    e.archive_clear()
    narrow = np.ascontiguousarray(arch[0, :64])
    assert e.lib.dne_archive_append(e.h, narrow.ctypes.data_as(C.POINTER(C.c_uint8)), 1, 64) == 0
    with pytest.raises(_lib.DneError, match=r"the archive holds entries of width 64, a RAM point has 128 bytes"):
        e.ram_novelty_pool(1, mem[:3])
    with pytest.raises(_lib.DneError, match=r"the archive holds entries of width 64"):
        e.archive_get_points(0, 1)
    assert e.archive_size() == 1
    e.archive_clear()
    # engines that keep no final RAM state per member: the NULL form and the gather
    for kw in (dict(record_bc=False), dict(record_bc=True, bc_max_steps=30)):
        kind = _lib.KIND_ES if kw.get("bc_max_steps") else _lib.KIND_GA
        other = _lib.Engine(kind, NACT, max_members=16, ref_count=16, **kw)
        try:
            text = "records full trajectories" if kw.get("bc_max_steps") else "created with record_bc = 0"
            with pytest.raises(_lib.DneError, match=text):
                other.ram_novelty_pool(1, n=2)
            with pytest.raises(_lib.DneError, match=text):
                other.archive_append_members([0])
            assert other.archive_size() == 0
            assert other.ram_novelty_pool(1, mem[:3]).shape == (3, )                                    # the host form needs no recorded state
        finally:
            other.close()
    # an index outside the last evaluation, and an append that would mix widths, on an engine that has evaluated
    ev = _lib.Engine(_lib.KIND_GA, NACT, max_members=16, record_bc=True)
    try:
        ev.noise_upload(G.noise_of(T.KIND_GA))
        ev.ga_set_init_scale(G.scale_by(T.KIND_GA))
        _, _, _, bc = ev.ga_eval_powers(_genomes(T.KIND_GA)[:4], 20, T.tap_seeds(4), want_bc=True)
        load(ev, arch[:3])
        for bad in ([0, 4], [-1], [2, 1, 9]):
            with pytest.raises(_lib.DneError, match=r"index \d is member -?\d, the last evaluation ran 4"):
                ev.archive_append_members(bad)
            assert ev.archive_size() == 3 and np.array_equal(ev.archive_get_points(0, 3), arch[:3])
        ev.archive_clear()
        assert ev.lib.dne_archive_append(ev.h, narrow.ctypes.data_as(C.POINTER(C.c_uint8)), 1, 64) == 0
        with pytest.raises(_lib.DneError, match=r"dne_archive_append: entry width 128, archive holds 64"):
            ev.archive_append_members([0])
        assert ev.archive_size() == 1
        ev.archive_clear()
        assert_same(pool(ev, 2), twin(bc, None, 2), "the recorded states survived every refusal")
    finally:
        ev.close()
    # the other kinds
    mz = _lib.Engine(_lib.KIND_MAZE, 2, max_members=16)
    dn = _lib.Engine(_lib.KIND_DENSE, 2, max_members=16, env=_lib.KIND_CARTPOLE, hidden=(), nonlin="relu")
    try:
        for other, name in ((mz, "DNE_KIND_MAZE"), (dn, "DNE_KIND_DENSE")):
            for call, args in ((other.ram_novelty_pool, (1, mem[:3])), (other.archive_append_members, ([0], )), (other.archive_get_points, (0, 1))):
                with pytest.raises(_lib.DneError, match=r"is not available on a %s engine" % name):
                    call(*args)
            assert other.ram_novelty_last_ms() == -1.0
    finally:
        mz.close(); dn.close()


# ---- 7. the driver ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ("prob_0.3", "prob_1_no_parents"))
def test_driver_on_the_device_equals_the_driver_on_the_host_engine(oracle, tmp_path, config):
    from dne_hip import _lib, ga_gpu
    import dense_support as D
    over = dict(ns={"archive_prob": 1.0}, selection_threshold=0) if config == "prob_1_no_parents" else {}
    exp = S.exp(**over)
    n = exp["population_size"]

    def run(log_dir, eng, iters):
        return ga_gpu.atari_ns_main(str(log_dir), engine=eng, noise=S.shared_noise(), seed=4, max_iters=iters, **exp)

    hip = _lib.Engine(_lib.KIND_GA, NACT, max_members=n, record_bc=True)
    try:
        a = run(tmp_path / "hip", hip, 2)
        b = run(tmp_path / "host", S.AtariGaNsHostEngine(max_members=n), 2)
        a = run(tmp_path / "hip", hip, 2)                                                               # the resume, on the same handle: the archive is pushed back
        b = run(tmp_path / "host", S.AtariGaNsHostEngine(max_members=n), 2)
        sa, sb = a[2], b[2]
        assert sa.it == sb.it == 4 and a[:2] == b[:2]
        assert [o.seeds for o in sa.population] == [o.seeds for o in sb.population] and [o.novelty for o in sa.population] == [o.novelty for o in sb.population]
        assert np.array_equal(sa.archive, sb.archive) and sa.timesteps_so_far == sb.timesteps_so_far and sa.elite.seeds == sb.elite.seeds
        assert np.array_equal(hip.archive_get_points(0, len(sa.archive)), sb.archive) if len(sb.archive) else hip.archive_size() == 0
        assert S.same_stream(sa.stream, sb.stream)
        assert D.log_rows(tmp_path / "hip") == D.log_rows(tmp_path / "host")
        assert hip.check_redzones() == 0
    finally:
        hip.close()
