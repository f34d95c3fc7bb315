"""The reference pass on unique operands (k_conv1_ref_uniq, k_bn1_gather, k_conv2_ref_uniq, k_y2_expand) against the oracle, bit for
bit: dne_get_bn_moments and the scale / shift of every member equal oracle.es_ref_pass_moments.  No tolerance anywhere.

16 reference frames, antithetic pairs at sigma 0.02 over the small noise table.  Every batch states its route and asserts it through
ref_dedup_support.expect_route (the engine's route and U1 / U2 against the host's index), so a test meant for the dedup kernels cannot pass
on the dense ones; under DNE_REF_DEDUP=0, set by hand for the whole suite, every batch here takes the dense kernels and must still equal
the oracle.  Batches:
  (a) the oracle's frames: the dedup route;
  (b) random bytes: nothing to share, the dense route;
  (c) sixteen flat frames (9 patches) and an all-zero batch (1 patch): tables shorter than one tile;
  (d) a batch whose U1 % 16 and U2 % 16 are both nonzero: both tables end inside a tile and inside a kernel's step;
  (e) 6 members at chunk size 4: a chunk boundary, two streams, a k_conv1_ref_uniq workgroup with dead member slots;
  (f) the largest tables that still fit (the oracle's frames with three frames of random bytes: 768 floats per member short of the end
      of the dense route's y1, less than one step of k_conv2_ref_uniq), 9 members at chunk size 8 (a full chunk, then a chunk of one on
      the second stream) and 4 at chunk size 4; both tables end in a workgroup segment shorter than steps_per_wg;
  (g) on one engine: (f), a batch one random frame longer (dense: it neither pays nor fits), the all-zero batch (dedup, one patch), (f)
      again -- the two layouts share the scratch, and rows a longer table left behind must not be read.
One short es_eval on batch (a) against the oracle: the lock-steps read what the pass left."""
import numpy as np
import pytest

import ref_dedup_support as S

pytestmark = pytest.mark.gpu

F, NACT, SIGMA = 16, 18, 0.02
IDX = np.array([12_345, 2_000_003, 777, 1_500_001, 31_337], np.int64)           # one noise offset per antithetic pair
MAX_MEMBERS = 12

_ENGINES = {}
_ORACLE = {}


@pytest.fixture(scope="module")
def hip(oracle):
    from dne_hip import _lib
    yield _lib
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear(); _ORACLE.clear()


def _engine(hip, noise, theta, ref_chunk, monkeypatch):
    """(engine, DNE_REF_DEDUP as it was created): one per chunk size and knob value"""
    knob = S.route_env(monkeypatch, "default")
    if (ref_chunk, knob) not in _ENGINES:
        e = hip.Engine(hip.KIND_ES, NACT, max_members=MAX_MEMBERS, ref_count=F, ref_chunk=ref_chunk)
        e.noise_upload(noise)
        e.set_theta(theta)
        _ENGINES[(ref_chunk, knob)] = e
    return _ENGINES[(ref_chunk, knob)], knob


def _theta(oracle):
    return oracle.es_init_theta(oracle.layout(oracle.KIND_ES, NACT), 0)


def _oracle_side(oracle, name, ref, noise, n):
    """(bn, moments) [n][608] of members 0..n-1 on the oracle, once per batch"""
    L = oracle.layout(oracle.KIND_ES, NACT)
    th = _theta(oracle)
    for i in range(n):
        if (name, i) not in _ORACLE:
            s = np.float32(SIGMA if i % 2 == 0 else -SIGMA)
            thi = th + s * noise[IDX[i // 2]:IDX[i // 2] + th.size]
            _ORACLE[(name, i)] = oracle.es_ref_pass_moments(L, thi, ref)
    return (np.stack([_ORACLE[(name, i)][0] for i in range(n)]), np.stack([_ORACLE[(name, i)][1] for i in range(n)]))


def _run(hip, oracle, noise, monkeypatch, name, ref, n, ref_chunk, want_dedup):
    """-> (U1, U2) of the batch on the host; expect_route holds the engine's to them wherever it has the tables"""
    e, knob = _engine(hip, noise, _theta(oracle), ref_chunk, monkeypatch)
    e.set_ref_batch(ref)
    route = S.expect_route(e, ref, knob, want_dedup)
    _, patches, _, windows, _ = hip.debug_ref_index(ref)
    U1, U2 = patches.shape[0], windows.shape[0]
    print("batch %s, %d members in chunks of %d: U1 = %d, U2 = %d, %s route (the engine reports U1, U2 = %r)"
          % (name, n, ref_chunk, U1, U2, route, e.ref_dedup_active()[1:]))
    off = np.repeat(IDX, 2)[:n]
    scale = np.array([SIGMA if i % 2 == 0 else -SIGMA for i in range(n)], np.float32)
    e.set_members(np.zeros(n, np.int32), off, scale)
    e.ref_pass(n)
    bn, mom = e.get_bn(n), e.get_bn_moments(n)
    obn, omom = _oracle_side(oracle, name, ref, noise, n)
    for i in range(n):
        assert np.array_equal(mom[i].view(np.int32), omom[i].view(np.int32)), (name, route, "moments of member", i)
        assert np.array_equal(bn[i].view(np.int32), obn[i].view(np.int32)), (name, route, "scale / shift of member", i)
    assert e.check_redzones() == 0
    return U1, U2


def test_fixture_frames_take_the_dedup_route(hip, oracle, small_noise, monkeypatch):
    _run(hip, oracle, small_noise, monkeypatch, "fixture", S.fixture_frames(F), 4, 8, True)


def test_random_frames_take_the_dense_route(hip, oracle, small_noise, monkeypatch):
    _run(hip, oracle, small_noise, monkeypatch, "random", S.random_frames(F), 4, 8, False)


def test_tables_below_one_tile(hip, oracle, small_noise, monkeypatch):
    U1, _ = _run(hip, oracle, small_noise, monkeypatch, "flat", S.flat_frames(F), 4, 8, True)
    assert U1 == 9
    U1, _ = _run(hip, oracle, small_noise, monkeypatch, "zero", np.zeros((F, 84, 84, 4), np.uint8), 4, 8, True)
    assert U1 == 1


def test_tables_that_end_inside_a_tile(hip, oracle, small_noise, monkeypatch):
    U1, U2 = _run(hip, oracle, small_noise, monkeypatch, "odd", S.odd_frames(F), 4, 8, True)
    assert U1 % 16 and U2 % 16


def test_chunk_boundary_and_dead_member_slots(hip, oracle, small_noise, monkeypatch):
    _run(hip, oracle, small_noise, monkeypatch, "fixture", S.fixture_frames(F), 6, 4, True)


def _k3_is_the_largest_that_fits(U1, U2):
    assert (U1, U2) == (4060, 1416)
    assert 0 <= S.room(F, U1, U2) == 768 < S.C2U_ROWS * 32            # y2u ends less than one k_conv2_ref_uniq step before the end of y1r
    assert (S.pad(U1, S.U1_PAD) // S.C1U_ROWS) % S.SPW1 and (S.pad(U2, S.U2_PAD) // S.C2U_ROWS) % S.SPW2   # short last segments


@pytest.mark.parametrize("n, ref_chunk", [(9, 8), (4, 4)])
def test_largest_tables_that_still_fit(hip, oracle, small_noise, monkeypatch, n, ref_chunk):
    """(9, 8): a full chunk whose y2u ends 8 * 768 floats before the end of its y1r, plus a chunk of one member on the second stream"""
    U1, U2 = _run(hip, oracle, small_noise, monkeypatch, "k3", S.mixed_frames(F, 3), n, ref_chunk, True)
    _k3_is_the_largest_that_fits(U1, U2)


def test_both_layouts_in_one_scratch(hip, oracle, small_noise, monkeypatch):
    """one engine, never recreated: the longest dedup tables, then the dense layout over the same floats, then the shortest tables (rows
    1 .. 4063 of y1u and of the patch table are what the batches before left there), then the longest again"""
    n, ref_chunk = 9, 8
    e = _engine(hip, small_noise, _theta(oracle), ref_chunk, monkeypatch)[0]
    _k3_is_the_largest_that_fits(*_run(hip, oracle, small_noise, monkeypatch, "k3", S.mixed_frames(F, 3), n, ref_chunk, True))
    U1, U2 = _run(hip, oracle, small_noise, monkeypatch, "k4", S.mixed_frames(F, 4), n, ref_chunk, False)
    assert (U1, U2) == (4428, 1498) and S.room(F, U1, U2) < 0
    U1, U2 = _run(hip, oracle, small_noise, monkeypatch, "zero", np.zeros((F, 84, 84, 4), np.uint8), n, ref_chunk, True)
    assert (U1, U2) == (1, 9)
    _run(hip, oracle, small_noise, monkeypatch, "k3", S.mixed_frames(F, 3), n, ref_chunk, True)
    assert _engine(hip, small_noise, _theta(oracle), ref_chunk, monkeypatch)[0] is e


def test_es_eval_behind_the_dedup_route(hip, oracle, small_noise, monkeypatch):
    ref = S.fixture_frames(F)
    e, knob = _engine(hip, small_noise, _theta(oracle), 8, monkeypatch)
    e.set_ref_batch(ref)
    print("es_eval on the fixture's frames: %s route" % S.expect_route(e, ref, knob, True))
    seeds = np.arange(4, dtype=np.uint32) + 1000
    ret, sg, ln = e.es_eval(IDX[:2], SIGMA, 8, seeds)
    oret, osg, oln = oracle.es_eval(oracle.layout(oracle.KIND_ES, NACT), _theta(oracle), small_noise, IDX[:2], SIGMA, 8, ref, seeds)
    assert np.array_equal(ln, oln) and np.array_equal(ret, oret) and np.array_equal(sg, osg), (ret, oret, ln, oln)
    assert e.check_redzones() == 0
