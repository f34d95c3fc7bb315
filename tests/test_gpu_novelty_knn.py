"""GPU: dne_novelty_knn -- k-NN novelty of a batch wholly on the device (tiled distance kernel + k-nearest selection),
bit for bit against the CPU oracle (orc_novelty: exact integer sums, the reference's three roundings, sort + ascending
sum).  Covers tile edges (archive and member counts around 64), lengths on every side of the archive's, k past the
archive, ties, 32-bit overflow, stale device rows, a large archive, archive updates, other widths and refusals."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NACT, NREF, BCMAX = 18, 16, 300


def oracle_all(archive, bcs, k):
    import oracle_pool
    return oracle_pool.novelty_all(archive, bcs, k)


@pytest.fixture(scope="module")
def eng(small_noise, oracle):
    from dne_hip import _lib
    e = _lib.Engine(_lib.KIND_ES, NACT, max_members=512, ref_count=NREF, record_bc=True, bc_max_steps=BCMAX)
    e.noise_upload(small_noise)
    ref = oracle.get_ref_batch(seed=0, batch_size=NREF, nact=NACT)
    e.set_ref_batch(ref)
    e.set_theta(oracle.es_init_theta(oracle.layout(0, NACT), 0))
    yield e, ref
    e.close()


def _ks(narch):
    return sorted({1, 10, max(narch - 1, 1), narch, narch + 5})


@pytest.mark.parametrize("narch,nmem", [(1, 1), (2, 7), (63, 64), (64, 65), (65, 200), (130, 7), (130, 65)])
def test_host_sets_against_oracle(eng, narch, nmem):
    e, _ = eng
    rs = np.random.RandomState(1000 * narch + nmem)
    alens = rs.randint(20, 61, narch)
    arch = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in alens]
    # 1 row, equal to an entry, shorter than every entry, longer than every entry, the recording capacity, random
    pick = [1, int(alens[0]), 7, 97, BCMAX]
    mlens = [pick[i] if i < len(pick) else int(rs.randint(1, 120)) for i in range(nmem)]
    bcs = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in mlens]
    for k in _ks(narch):
        got = e.novelty_knn(arch, k, bcs=bcs)
        assert np.array_equal(got, oracle_all(arch, bcs, k)), (narch, nmem, k)


def test_ties_and_identical_entry(eng, oracle):
    e, _ = eng
    rs = np.random.RandomState(5)
    bcs = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in (9, 30, 1)]
    base = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in (4, 30, 12)]
    arch = base + [base[0].copy(), base[1].copy(), base[1].copy(), bcs[1].copy()]   # duplicates; an entry equal to member 1
    for k in (1, 2, 3, 5, 7, 12):
        got = e.novelty_knn(arch, k, bcs=bcs)
        assert np.array_equal(got, np.array([oracle.novelty(arch, b, k) for b in bcs])), k
    assert e.novelty_knn(arch, 1, bcs=bcs)[1] == 0.0


def test_extremes_no_32bit_overflow(eng, oracle):
    e, _ = eng
    hi_long = np.full((5000, 128), 255, np.uint8)
    lo_one = np.zeros((1, 128), np.uint8)
    A, B = 128 * 255 ** 2, 4999 * 128 * 255 ** 2      # B alone is past 2^32
    a, b = math.sqrt(A), math.sqrt(B)
    closed = math.sqrt(a * a + b * b)
    assert e.novelty_knn([lo_one], 1, bcs=[hi_long])[0] == closed == oracle.novelty([lo_one], hi_long, 1)
    assert e.novelty_knn([hi_long], 1, bcs=[lo_one])[0] == closed == oracle.novelty([hi_long], lo_one, 1)
    both = e.novelty_knn([lo_one, hi_long], 2, bcs=[hi_long, lo_one])
    assert np.array_equal(both, [oracle.novelty([lo_one, hi_long], hi_long, 2), oracle.novelty([lo_one, hi_long], lo_one, 2)])


def test_recorded_after_longer_run(eng, oracle, small_noise):
    """the trajectories kept on the device (bcs = NULL): rows past a member's length hold a longer earlier run's data"""
    e, _ = eng
    rs = np.random.RandomState(7)
    P = e.P
    idx1 = rs.randint(0, small_noise.size - P + 1, 256).astype(np.int64)
    idx2 = rs.randint(0, small_noise.size - P + 1, 256).astype(np.int64)
    s1 = rs.randint(0, 2 ** 32, 512, dtype=np.uint64).astype(np.uint32)
    s2 = rs.randint(0, 2 ** 32, 512, dtype=np.uint64).astype(np.uint32)
    e.es_eval(idx1, 0.02, 60, s1)                                # fills more rows than the next run reads
    _, _, ln = e.es_eval(idx2, 0.02, 25, s2)
    ln = ln.reshape(-1)
    arch = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in rs.randint(1, 90, 100)]
    k = 10
    got = e.novelty_knn(arch, k, lengths=ln)
    batch = e.novelty_batch(arch, ln, k)
    _, _, ln_b, bc = e.es_eval(idx2, 0.02, 25, s2, want_bc=True)   # same evaluation again, trajectories downloaded
    assert np.array_equal(ln_b.reshape(-1), ln)
    bc = bc.reshape(512, BCMAX, 128)
    bcs = [bc[i, :ln[i]] for i in range(512)]
    want = oracle_all(arch, bcs, k)
    assert np.array_equal(got, want) and np.array_equal(batch, want)


def test_scale_archive_1024(eng):
    e, _ = eng
    rs = np.random.RandomState(11)
    arch = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in rs.randint(1, 2001, 1024)]
    bcs = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in rs.randint(1, 600, 256)]
    got = e.novelty_knn(arch, 10, bcs=bcs)
    assert np.array_equal(got, oracle_all(arch, bcs, 10))


def test_archive_append_clear_and_one_shot(eng, oracle):
    from dne_hip import _lib
    e, _ = eng
    rs = np.random.RandomState(13)
    bcs = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in (5, 40, 17)]
    arch = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in (10, 30)]
    want = lambda a, k: np.array([oracle.novelty(a, b, k) for b in bcs])
    assert np.array_equal(e.novelty_knn(arch, 2, bcs=bcs), want(arch, 2))
    for n in (3, 50, 70):                                         # appended between calls (same objects: uploads only the new entry)
        arch = arch + [rs.randint(0, 256, (n, 128)).astype(np.uint8)]
        assert np.array_equal(e.novelty_knn(arch, 3, bcs=bcs), want(arch, 3))
    short = [arch[2].copy()]                                      # a different list: cleared and uploaded again
    assert np.array_equal(e.novelty_knn(short, 3, bcs=bcs), want(short, 3))
    # the one-shot form of dne_novelty replaces the resident archive; dne_novelty_knn then scores against it
    one = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in (8, 9, 60)]
    flat = np.ascontiguousarray(np.concatenate(one))
    alen = np.array([a.shape[0] for a in one], np.int32)
    out = C.c_double()
    assert e.lib.dne_novelty(e.h, _lib._ptr(flat, C.c_uint8), _lib._ptr(alen, C.c_int32), 3, _lib._ptr(bcs[0], C.c_uint8),
                             int(bcs[0].shape[0]), 128, 2, C.byref(out)) == 0
    assert out.value == oracle.novelty(one, bcs[0], 2)
    rows = np.ascontiguousarray(np.concatenate(bcs))
    ln = np.array([b.shape[0] for b in bcs], np.int32)
    got = np.empty(3, np.float64)
    assert e.lib.dne_novelty_knn(e.h, _lib._ptr(rows, C.c_uint8), _lib._ptr(ln, C.c_int32), 3, 128, 2, _lib._ptr(got, C.c_double)) == 0
    assert np.array_equal(got, want(one, 2))
    e.lib.dne_archive_clear(e.h)
    e._arch_objs = []


@pytest.mark.parametrize("dim", [3, 7, 64, 200])
def test_other_widths(eng, oracle, dim):
    e, _ = eng
    rs = np.random.RandomState(dim)
    arch = [rs.randint(0, 256, (n, dim)).astype(np.uint8) for n in (1, 6, 33, 90)]
    bcs = [rs.randint(0, 256, (n, dim)).astype(np.uint8) for n in (1, 6, 20, 120)]
    for k in (1, 3, 9):
        for b in bcs:
            assert e.novelty(arch, b, k) == oracle.novelty(arch, b, k)    # dne_novelty: the n = 1 host form
        assert np.array_equal(e.novelty_knn(arch, k, bcs=bcs), np.array([oracle.novelty(arch, b, k) for b in bcs]))


def test_refusals_leave_the_device_usable(eng, oracle):
    from dne_hip import _lib
    e, _ = eng
    rs = np.random.RandomState(17)
    arch = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in (4, 9)]
    bcs = [rs.randint(0, 256, (n, 128)).astype(np.uint8) for n in (3, 12)]
    with pytest.raises(_lib.DneError):
        e.novelty_knn(arch, 0, bcs=bcs)                                                    # k < 1
    with pytest.raises(_lib.DneError):
        e.novelty_knn([], 1, bcs=bcs)                                                      # empty archive
    with pytest.raises(_lib.DneError):
        e.novelty_knn(arch, 1, bcs=[b[:, :64] for b in bcs])                               # width mismatch
    with pytest.raises(_lib.DneError):
        e.novelty_knn(arch, 1, bcs=[bcs[0], bcs[1][:0]])                                   # a trajectory of 0 rows
    with pytest.raises(_lib.DneError):
        e.novelty_knn(arch, 1, lengths=np.array([3, BCMAX + 1], np.int32))                 # past the recorded capacity
    with pytest.raises(_lib.DneError):
        e.novelty_knn(arch, 1, lengths=np.array([0, 3], np.int32))
    with pytest.raises(_lib.DneError):
        e.novelty_knn(arch, 1, lengths=np.ones(513, np.int32))                             # more members than recorded
    assert np.array_equal(e.novelty_knn(arch, 2, bcs=bcs), np.array([oracle.novelty(arch, b, 2) for b in bcs]))
