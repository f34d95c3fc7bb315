"""The reference pass on unique operands (k_conv1_ref_uniq, k_bn1_gather, k_conv2_ref_uniq, k_y2_expand) against the oracle, bit for
bit: dne_get_bn_moments and the scale / shift of every member equal oracle.es_ref_pass_moments.  No tolerance anywhere.

16 reference frames, two antithetic pairs at sigma 0.02 over the small noise table.  Batches:
  (a) the oracle's frames: the dedup route (asserted through dne_ref_dedup_active, so the test cannot pass on the dense kernels);
  (b) random bytes: nothing to share, the dense route;
  (c) sixteen flat frames (9 patches) and an all-zero batch (1 patch): tables shorter than one tile;
  (d) a batch whose U1 % 16 and U2 % 16 are both nonzero: both tables end inside a tile and inside a kernel's step;
  (e) 6 members at chunk size 4: a chunk boundary, two streams, a k_conv1_ref_uniq workgroup with dead member slots.
One short es_eval on batch (a) against the oracle: the lock-steps read what the pass left."""
import numpy as np
import pytest

import ref_dedup_support as S

pytestmark = pytest.mark.gpu

F, NACT, SIGMA = 16, 18, 0.02
IDX = np.array([12_345, 2_000_003, 777], np.int64)           # one noise offset per antithetic pair

_ENGINES = {}
_ORACLE = {}


@pytest.fixture(scope="module")
def hip(oracle):
    from dne_hip import _lib
    yield _lib
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear(); _ORACLE.clear()


def _engine(hip, noise, theta, ref_chunk):
    if ref_chunk not in _ENGINES:
        e = hip.Engine(hip.KIND_ES, NACT, max_members=8, ref_count=F, ref_chunk=ref_chunk)
        e.noise_upload(noise)
        e.set_theta(theta)
        _ENGINES[ref_chunk] = e
    return _ENGINES[ref_chunk]


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


def _run(hip, oracle, noise, name, ref, n, ref_chunk, want_dedup):
    e = _engine(hip, noise, _theta(oracle), ref_chunk)
    e.set_ref_batch(ref)
    dedup, U1, U2 = e.ref_dedup_active()
    print("batch %s: U1 = %d, U2 = %d, %s route" % (name, U1, U2, "dedup" if dedup else "dense"))
    assert dedup == want_dedup
    off = np.repeat(IDX, 2)[:n]
    scale = np.array([SIGMA if i % 2 == 0 else -SIGMA for i in range(n)], np.float32)
    e.set_members(np.zeros(n, np.int32), off, scale)
    e.ref_pass(n)
    bn, mom = e.get_bn(n), e.get_bn_moments(n)
    obn, omom = _oracle_side(oracle, name, ref, noise, n)
    for i in range(n):
        assert np.array_equal(mom[i].view(np.int32), omom[i].view(np.int32)), (name, "moments of member", i)
        assert np.array_equal(bn[i].view(np.int32), obn[i].view(np.int32)), (name, "scale / shift of member", i)
    assert e.check_redzones() == 0
    return U1, U2


def test_fixture_frames_take_the_dedup_route(hip, oracle, small_noise):
    _run(hip, oracle, small_noise, "fixture", S.fixture_frames(F), 4, 8, True)


def test_random_frames_take_the_dense_route(hip, oracle, small_noise):
    _run(hip, oracle, small_noise, "random", S.random_frames(F), 4, 8, False)


def test_tables_below_one_tile(hip, oracle, small_noise):
    U1, _ = _run(hip, oracle, small_noise, "flat", S.flat_frames(F), 4, 8, True)
    assert U1 == 9
    U1, _ = _run(hip, oracle, small_noise, "zero", np.zeros((F, 84, 84, 4), np.uint8), 4, 8, True)
    assert U1 == 1


def test_tables_that_end_inside_a_tile(hip, oracle, small_noise):
    U1, U2 = _run(hip, oracle, small_noise, "odd", S.odd_frames(F), 4, 8, True)
    assert U1 % 16 and U2 % 16


def test_chunk_boundary_and_dead_member_slots(hip, oracle, small_noise):
    _run(hip, oracle, small_noise, "fixture", S.fixture_frames(F), 6, 4, True)


def test_es_eval_behind_the_dedup_route(hip, oracle, small_noise):
    ref = S.fixture_frames(F)
    e = _engine(hip, small_noise, _theta(oracle), 8)
    e.set_ref_batch(ref)
    assert e.ref_dedup_active()[0]
    seeds = np.arange(4, dtype=np.uint32) + 1000
    ret, sg, ln = e.es_eval(IDX[:2], SIGMA, 8, seeds)
    oret, osg, oln = oracle.es_eval(oracle.layout(oracle.KIND_ES, NACT), _theta(oracle), small_noise, IDX[:2], SIGMA, 8, ref, seeds)
    assert np.array_equal(ln, oln) and np.array_equal(ret, oret) and np.array_equal(sg, osg), (ret, oret, ln, oln)
    assert e.check_redzones() == 0
