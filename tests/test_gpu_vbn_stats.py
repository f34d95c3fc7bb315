"""The reference pass (dne_ref_pass: the scale / shift every ES and ModelVirtualBN step kernel applies) on the GPU, every member:

  * get_bn / get_bn_moments equal the oracle bit for bit;
  * the engine's moments lie within the float64 tolerances of tests/vbn_stats_support.py around float64 moments of the layer outputs
    (oracle.forward_debug over every reference frame, fed with the engine's own bn: the bn asserted bit-equal to the oracle's one line
    earlier, which is why the float64 side can be computed before the engine runs and shared between tests);
  * the engine's bn is scale_shift32 of the engine's own moments, bit for bit;
  * act on a reference frame and on random bytes: logits and every layer's output equal the oracle's, so the scale of a clamped
    variance (gamma / sqrt(1e-3)) is also seen through a consumer;
  * no kernel wrote outside its buffer.

Inputs: the cases of vbn_stats_support (perturbed start point; ill-conditioned theta on the fixture's frames, on all-zero, all-255 and
repeated-frame batches; 254 / 255 noise under one-tap channels, where rounding engages the variance clamp) at 8 (generic fc path), 16 and
128 (matrix-core fc, one and two frame groups) reference frames, on an ES and a ModelVirtualBN engine; 12 members = two chunks of the
engine's ref_chunk = 8 on two streams, with scales from {0.02, -0.02, 0, 0.5} (the scale-0 members are the case's theta itself).

Routes: at 16 and 128 frames the engine has two sets of convolution kernels for the pass and picks per batch (csrc/ref_index.h); every
test here runs both -- "default" (the engine's pick: the unique-row kernels for cases a to e, the dense ones for f, asserted) and "dense"
(DNE_REF_DEDUP=0: k_conv1_ref_shared<16> and k_conv2_ref<16, true> on every batch, the degenerate ones included) -- against the same
expected side, states the route it ran (ref_dedup_support.expect_route) and prints it.  8 frames have one route.

Chunking: one chunk, a last chunk of one member (seven phantom members in k_fc_ref's eight-member grid), three chunks (a scratch set is
used twice), three full chunks, and a chunk size that is no multiple of 8.

tests/test_vbn_stats_cpu.py shows on the CPU that the assertion used here reports a wrong count, a bias counted twice, a missing clamp, a
dropped tile or frame, unbiased variance and a wrong epsilon."""
import multiprocessing as mp

import numpy as np
import pytest

import ref_dedup_support as S
import vbn_stats_support as V
from vbn_stats_support import CASES, FS, KINDS, NACT

pytestmark = pytest.mark.gpu

N_MAIN = 12
SCALES = (0.02, -0.02, 0.0, 0.5)
MAX_MEMBERS = 24

_BASE = None
_REFS = {}       # (kind, case, F, member) -> the oracle / float64 side of one member
_ENGINES = {}    # (kind, F, ref_chunk, DNE_REF_DEDUP) -> Engine
_EVALS = {}      # (kind, batch) -> the oracle's side of test_es_eval_on_degenerate_reference_batches
# the route dne_set_ref_batch picks for each case's batch on the default knobs, at 16 and at 128 frames alike (the model cost of
# csrc/ref_index.h against the dense kernels' 29.76: a, b 25.27 / 12.15; c 5.1; d 5.2; e 6.9 / 5.3; f 42.85 -- every row distinct)
DEDUP_BY_DEFAULT = dict(a=True, b=True, c=True, d=True, e=True, f=False)


@pytest.fixture(scope="module")
def hip():
    from dne_hip import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _close_engines(oracle):
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear(); _REFS.clear(); _EVALS.clear()


def _P(kind):
    import vbn_support
    return V.layout().P if kind == "es" else vbn_support.layouts(NACT)[0][1]


def _base_theta(kind, case, F):
    """the case's theta in the engine kind's own layout"""
    import vbn_support
    th = V.case_inputs(case, F)[0]
    return th if kind == "es" else vbn_support.contract(th, NACT)


def _members(kind, noise):
    """24 members, the same for every case: noise offsets (member 1 is member 0's antithetic twin) and scales"""
    off = np.random.RandomState(5).randint(0, noise.size - _P(kind), MAX_MEMBERS).astype(np.int64)
    off[1] = off[0]
    return off, np.array([SCALES[i % 4] for i in range(MAX_MEMBERS)], np.float32)


def _member_theta(kind, base, noise, off, scale, i):
    """member i's vector in the ES layout, as the oracle runs it"""
    import vbn_support
    thi = base + np.float32(scale[i]) * noise[off[i]:off[i] + base.size]
    return thi if kind == "es" else vbn_support.expand(thi, NACT)


def _observations(case, F):
    ref = V.case_inputs(case, F)[1]
    return np.stack([ref[F // 2], np.random.RandomState(77).randint(0, 256, (84, 84, 4)).astype(np.uint8)])


def _member_job(i):
    import oracle as O
    kind, base, noise, off, scale, ref, obs = _BASE
    L = V.layout()
    th = _member_theta(kind, base, noise, off, scale, i)
    bn, mom = O.es_ref_pass_moments(L, th, ref)
    ref64, _ = V.reference_moments(L, th, ref, bn)
    return dict(bn=bn, mom=mom, ref64=ref64, fwd=[O.forward_debug(L, th, bn, ob) for ob in obs])


def _refs(kind, case, F, n, noise):
    """the oracle's reference pass, the float64 moments and the two forward passes of members 0..n-1, computed once per member over the
    host's cores (at most 16) and kept for every test that needs them"""
    global _BASE
    import oracle_pool
    todo = [i for i in range(n) if (kind, case, F, i) not in _REFS]
    if todo:
        off, scale = _members(kind, noise)
        _BASE = (kind, _base_theta(kind, case, F), noise, off, scale, V.case_inputs(case, F)[1], _observations(case, F))
        try:
            with mp.get_context("fork").Pool(min(oracle_pool.workers(), 16, len(todo))) as pool:
                for i, r in zip(todo, pool.map(_member_job, todo, chunksize=1)):
                    _REFS[(kind, case, F, i)] = r
        finally:
            _BASE = None
    return [_REFS[(kind, case, F, i)] for i in range(n)]


def _engine(hip, kind, F, ref_chunk, noise, route, monkeypatch):
    """(engine, DNE_REF_DEDUP as it was created); the knobs are read once in dne_create, so the environment is set first"""
    knob = S.route_env(monkeypatch, route)
    key = (kind, F, ref_chunk, knob)
    if key not in _ENGINES:
        e = hip.Engine(hip.KIND_ES if kind == "es" else hip.KIND_ES_VBN, NACT, max_members=MAX_MEMBERS, ref_count=F, ref_chunk=ref_chunk)
        e.noise_upload(noise)
        _ENGINES[key] = e
    return _ENGINES[key], knob


def _run_ref_pass(e, knob, route, kind, case, F, n, noise):
    off, scale = _members(kind, noise)
    e.set_theta(_base_theta(kind, case, F))
    ref = V.case_inputs(case, F)[1]
    e.set_ref_batch(ref)
    ran = S.expect_route(e, ref, knob, DEDUP_BY_DEFAULT[case])
    print("%s case %s F=%d n=%d, route asked for: %s -> %s kernels" % (kind, case, F, n, route, ran))
    e.set_members(np.zeros(n, np.int32), off[:n], scale[:n])
    e.ref_pass(n)
    return e.get_bn(n), e.get_bn_moments(n)


def _check_members(kind, case, F, n, noise, bn, mom, refs):
    L = V.layout()
    off, scale = _members(kind, noise)
    base = _base_theta(kind, case, F)
    worst = {}
    for i in range(n):
        r = refs[i]
        assert np.array_equal(bn[i].view(np.int32), r["bn"].view(np.int32)), (kind, case, F, n, "bn of member", i)
        assert np.array_equal(mom[i].view(np.int32), r["mom"].view(np.int32)), (kind, case, F, n, "moments of member", i)
        th = _member_theta(kind, base, noise, off, scale, i)
        for k, v in V.check_statistics(L, th, F, bn[i], mom[i], r["ref64"]).items():
            worst[k] = max(v, worst.get(k, 0.0))
    print("%s case %s F=%d n=%d worst observed / tolerance: " % (kind, case, F, n) + "  ".join("%s/%s %.4f" % (k + (v,)) for k, v in sorted(worst.items())))
    return worst


@pytest.mark.parametrize("kind, case, F, route", [pytest.param(kind, case, F, route, id="%s-%s-%d%s" % (kind, case, F, S.route_id(route)))
                                                  for kind in KINDS for case in CASES for F in FS for route in S.routes(F)])
def test_ref_pass_statistics_every_member(hip, small_noise, monkeypatch, kind, case, F, route):
    n = N_MAIN
    refs = _refs(kind, case, F, n, small_noise)
    e, knob = _engine(hip, kind, F, 8, small_noise, route, monkeypatch)
    bn, mom = _run_ref_pass(e, knob, route, kind, case, F, n, small_noise)
    _check_members(kind, case, F, n, small_noise, bn, mom, refs)
    if case == "c":       # conv1 of an all-zero batch: every variance exactly 0, the clamped scale gamma / sqrt(1e-3) in every member
        assert not mom[:, 16:32].any()
    if case == "f" and kind == "es":   # the clamp engaged by rounding, in the members that are the case's theta itself
        for i in range(2, n, 4):
            assert mom[i, 16 + V.F_CLAMP[F]] == 0
    obs = _observations(case, F)
    for k in range(2):
        e.env_set_observation(np.repeat(obs[k:k + 1], n, axis=0))
        acts, logits = e.act(n)
        for i in range(n):
            y1, y2, y3, lg = refs[i]["fwd"][k]
            g1, g2, g3 = e.debug_activations(i)
            assert np.array_equal(g1, y1) and np.array_equal(g2, y2) and np.array_equal(g3, y3), (kind, case, F, k, i)
            assert np.array_equal(logits[i], lg), (kind, case, F, k, i)
            assert acts[i] == int(np.argmax(lg)), (kind, case, F, k, i)     # np.argmax: the first maximum, the contract's argmax
    assert e.check_redzones() == 0


# ref_chunk, member counts: one chunk on one stream; a last chunk of one member; three chunks (the first scratch set used twice); three full
# chunks; a chunk size that is no multiple of k_fc_ref's eight-member grid
CHUNKING = [(8, 8), (8, 9), (8, 17), (8, 24), (5, 11)]


@pytest.mark.parametrize("kind, F, ref_chunk, n, route", [pytest.param(kind, F, ref_chunk, n, route, id="%s-%d-%d-%d%s" % (kind, F, ref_chunk, n, S.route_id(route)))
                                                          for kind in KINDS for F in (128, 8) for ref_chunk, n in CHUNKING for route in S.routes(F)])
def test_ref_pass_chunking_every_member(hip, small_noise, monkeypatch, kind, F, ref_chunk, n, route):
    """case b: at F = 128 the dedup kernels ("default") and the dense ones ("dense": k_conv1_ref_shared<16>, whose (nc + 7) / 8 workgroups
    have dead member slots of their own, k_conv2_ref<16, true>), at F = 8 the generic path"""
    case = "b"
    refs = _refs(kind, case, F, n, small_noise)
    e, knob = _engine(hip, kind, F, ref_chunk, small_noise, route, monkeypatch)
    bn, mom = _run_ref_pass(e, knob, route, kind, case, F, n, small_noise)
    _check_members(kind, case, F, n, small_noise, bn, mom, refs)
    assert e.check_redzones() == 0


@pytest.mark.parametrize("kind, batch, route", [pytest.param(kind, batch, route, id="%s-%s%s" % (kind, batch, S.route_id(route)))
                                                for kind in KINDS for batch in ("zero", "repeated") for route in S.ROUTES])
def test_es_eval_on_degenerate_reference_batches(hip, oracle, small_noise, monkeypatch, kind, batch, route):
    """two antithetic pairs, three steps, under batch statistics whose conv1 variances are all exactly zero (all-zero frames) or whose fc
    variances are rounding noise (one frame repeated): the step kernels apply the same clamped scales as the oracle"""
    import vbn_support
    O = oracle
    F = 16
    th_es, ref = V.case_inputs("c" if batch == "zero" else "e", F)
    base = _base_theta(kind, "c", F)
    P = base.size
    idx = np.array([12_345, small_noise.size - P], np.int64)
    seeds = np.array([3, 1_000_003, 77, 2 ** 31 + 5], np.uint32)
    sigma, tslimit = 0.02, 3
    if (kind, batch) not in _EVALS:
        if kind == "es":
            _EVALS[(kind, batch)] = O.es_eval(V.layout(), base, small_noise, idx, sigma, tslimit, ref, seeds)
        else:
            _EVALS[(kind, batch)] = vbn_support.es_pairs(small_noise, base, ref, idx, seeds, sigma, tslimit, NACT)[:3]
    oret, osg, oln = _EVALS[(kind, batch)]
    knob = S.route_env(monkeypatch, route)
    e = hip.Engine(hip.KIND_ES if kind == "es" else hip.KIND_ES_VBN, NACT, max_members=4, ref_count=F)
    try:
        e.noise_upload(small_noise)
        e.set_theta(base)
        e.set_ref_batch(ref)
        print("%s %s batch, route asked for: %s -> %s kernels" % (kind, batch, route, S.expect_route(e, ref, knob, True)))
        ret, sg, ln = e.es_eval(idx, sigma, tslimit, seeds)
        assert np.array_equal(ln, oln) and np.array_equal(ret, oret) and np.array_equal(sg, osg), (ret, oret, ln, oln)
        assert (ln == tslimit).all()
        assert e.check_redzones() == 0
    finally:
        e.close()
