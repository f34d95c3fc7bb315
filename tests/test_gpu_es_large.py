"""GPU: the ES loop of the GPU tree over its LargeModel (gpu_implementation/es.py:144 takes exp['model'] from any of its models) -- dne_es_eval on a
DNE_KIND_GA_LARGE engine: antithetic pairs over base slot 0, no reference pass, the streamed fc sharing a pair's theta and noise rows
(csrc/forward_large.h: k_lfc_pair).  Checked against the oracle (perturb + rollout per member, forward_large_debug for the kernels' own sums), against
the engine's second route through the per-member kernels (set_members + eval_members), through dne_es_update, the wire records, the es_gpu.py driver
and in alternation with Deep-GA generations on one engine.

The fixture: five pairs whose episodes under tslimit 200 end at different times (the oracle's lengths are asserted before the engine is looked at)."""
import functools

import numpy as np
import pytest

import step_tap_support as S

pytestmark = pytest.mark.gpu
NACT = 18
SIGMA, TSLIMIT = 0.02, 200
IDX = np.array([4947342, 99, 555, 17, 2222222], np.int64)          # the first is the last legal slice: 4947342 + P = 9 000 000
SEEDS = np.array([29, 30, 33, 34, 21, 22, 27, 28, 25, 26], np.uint32)
ORACLE_LENGTHS = [[118, 169], [200, 137], [200, 200], [200, 200], [200, 200]]
TAPS = (1, 3, 9)
PAIR = {"DNE_LFC_COLS_MAX": "0"}                                   # k_lfc_pair at every count


def _O():
    import oracle as O
    O.build()
    return O


@functools.lru_cache(maxsize=None)
def scale_by():
    from dne_hip import _lib, ga_gpu
    return ga_gpu.model_scale_by(NACT, _lib.KIND_GA_LARGE)


@functools.lru_cache(maxsize=None)
def theta():
    P = S.num_params(S.KIND_GA_LARGE)
    assert IDX[0] + P == S.LARGE_NOISE_LEN
    return (S.big_noise()[1234:1234 + P] * scale_by()).astype(np.float32)


def member_theta(idx, sign, sigma=SIGMA):
    return _O().perturb(theta(), S.big_noise(), idx, sigma, sign)


@functools.lru_cache(maxsize=None)
def oracle_eval():
    """returns, sign-returns, lengths [5][2] of the fixture: perturb + rollout per member (the oracle's es_eval wrapper wants a reference array)"""
    O = _O()
    L = O.layout(O.KIND_GA_LARGE, NACT)
    ret = np.zeros((5, 2), np.float32); sg = np.zeros((5, 2), np.float32); ln = np.zeros((5, 2), np.int32)
    for i in range(5):
        for s in range(2):
            ret[i, s], sg[i, s], ln[i, s] = O.rollout(L, member_theta(IDX[i], 1 if s == 0 else -1), None, SEEDS[2 * i + s], TSLIMIT)[:3]
    # what the fixture is for, held on the oracle's own lengths: a change of fixture cannot quietly stop exercising these
    lens = ln.tolist()
    assert lens == ORACLE_LENGTHS
    burst = 16                                                         # DNE_BURST_TAIL: ten members compact every 16 lock-steps
    assert any(abs(a - b) > 2 * burst and max(a, b) < TSLIMIT for a, b in lens)          # one member gone long before the other, across compactions
    assert any(a == TSLIMIT and b < TSLIMIT for a, b in lens)                            # a pair that loses its second member only
    assert any(max(a, b) < TSLIMIT and max(a, b) % burst != 0 for a, b in lens)          # wholly finished, in the list until the next compaction
    assert len(lens) % 2 == 1
    return ret, sg, ln


@functools.lru_cache(maxsize=None)
def oracle_taps(i, s):
    O = _O()
    L = O.layout(O.KIND_GA_LARGE, NACT)
    return S.oracle_taps(L, member_theta(IDX[i], 1 if s == 0 else -1), None, int(SEEDS[2 * i + s]), TAPS, large=True)


def make_engine(monkeypatch, knobs, max_members=10, theta_vec=None):
    from dne_hip import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    e = _lib.Engine(_lib.KIND_GA_LARGE, NACT, max_members=max_members)
    e.noise_upload(S.big_noise())
    e.ga_set_init_scale(scale_by())
    e.set_theta(theta() if theta_vec is None else theta_vec)
    return e


_CROSS = [pytest.param(dict(PAIR, DNE_FC_RB=rb, DNE_NSUB=ns, **grid), 6, id="pair-rb%s-nsub%s%s" % (rb, ns, "-grid1" if grid else ""))
          for rb in ("4", "8") for ns in ("1", "2") for grid in ({}, {"DNE_FC_GRID": "1"})]


@pytest.mark.parametrize("knobs,kind", _CROSS + [pytest.param({}, 1, id="default-cols")])
def test_whole_evaluation_equals_the_oracle(knobs, kind, monkeypatch):
    oret, osg, oln = oracle_eval()
    e = make_engine(monkeypatch, knobs)
    try:
        ret, sg, ln = e.es_eval(IDX, SIGMA, TSLIMIT, SEEDS)
        print("lengths", ln.tolist(), "returns", ret.tolist())
        assert np.array_equal(ln, oln) and np.array_equal(ret, oret) and np.array_equal(sg, osg), (ln, oln, ret, oret)
        assert e.profile()["fc_full_kind"] == kind
        assert e.check_redzones() == 0
    finally:
        e.close()


def test_route_identity(monkeypatch):
    """the same ten members as groups of one on the per-member kernels: bit-identical to the pairs of es_eval"""
    e = make_engine(monkeypatch, PAIR)
    try:
        ret, sg, ln = e.es_eval(IDX, SIGMA, TSLIMIT, SEEDS)
        assert e.profile()["fc_full_kind"] == 6
        e.set_members(np.zeros(10, np.int32), np.repeat(IDX, 2), np.tile(np.array([SIGMA, -SIGMA], np.float32), 5))
        r2, s2, l2 = e.eval_members(10, TSLIMIT, SEEDS)
        assert e.profile()["fc_full_kind"] == 1
        assert np.array_equal(l2, ln.reshape(-1)) and np.array_equal(r2, ret.reshape(-1)) and np.array_equal(s2, sg.reshape(-1))
        assert np.array_equal(ln, oracle_eval()[2])
        assert e.check_redzones() == 0
    finally:
        e.close()


@pytest.mark.parametrize("rb", ["4", "8"])
def test_taps(rb, monkeypatch):
    """y1 .. y4 of every member after es_eval at T = 1, 3, 9 against forward_large_debug on the oracle's observation of that step: the kernel's
    sums themselves, not only their argmax (DNE_BURST=4: T = 9 lies behind two compactions)"""
    e = make_engine(monkeypatch, dict(PAIR, DNE_FC_RB=rb, DNE_BURST="4", DNE_BURST_TAIL="4"))
    try:
        for T in TAPS:
            ret, sg, ln = e.es_eval(IDX, SIGMA, T, SEEDS)
            assert e.profile()["fc_full_kind"] == 6 and (ln == T).all()
            for i in range(5):
                for s in range(2):
                    tap = oracle_taps(i, s)[T]
                    assert (ret[i, s], sg[i, s], ln[i, s]) == (tap["ret"], tap["sign"], tap["length"]), (T, i, s)
                    for name, got, want in zip(("y1", "y2", "y3", "y4"), e.debug_activations_large(2 * i + s), tap["y"]):
                        assert np.array_equal(got, want), (T, i, s, name, int((got != want).sum()))
        assert e.check_redzones() == 0
    finally:
        e.close()


def test_default_routing_at_width(monkeypatch):
    """100 pairs under the default knobs: two windows of 50 pairs = 100 members each, above lfc_cols_max -> k_lfc_pair without any knob"""
    from dne_hip import _lib
    O = _O()
    L = O.layout(O.KIND_GA_LARGE, NACT)
    n, T = 100, 3
    rs = np.random.RandomState(100)
    idx = rs.randint(0, S.LARGE_NOISE_LEN - L.P + 1, n).astype(np.int64)
    idx[0], idx[-1] = 0, S.LARGE_NOISE_LEN - L.P
    seeds = S.tap_seeds(2 * n)
    rows = _lib.debug_plan(_lib.KIND_GA_LARGE, NACT, n, 2, antithetic_slot0=1, uniform_base=1)
    assert [(r.cnt, _lib.FC_NAMES[r.fc]) for r in rows] == [(50, "k_lfc_pair")] * 2
    e = make_engine(monkeypatch, {}, max_members=2 * n)
    try:
        ret, sg, ln = e.es_eval(idx, SIGMA, T, seeds)
        assert e.profile()["fc_full_kind"] == 6
        pick = sorted({0, 2 * n - 1} | set(rs.permutation(2 * n)[:4].tolist()))
        for m in range(2 * n):
            th = member_theta(idx[m // 2], 1 if m % 2 == 0 else -1)
            if m in pick:
                tap = S.oracle_taps(L, th, None, int(seeds[m]), (T,), large=True)[T]
                assert np.array_equal(e.debug_activations_large(m)[3], tap["y"][3]), m
                want = (tap["ret"], tap["sign"], tap["length"])
            else:
                want = O.rollout(L, th, None, seeds[m], T)[:3]
            assert (ret[m // 2, m % 2], sg[m // 2, m % 2], ln[m // 2, m % 2]) == want, m
        assert e.check_redzones() == 0
    finally:
        e.close()


@pytest.mark.parametrize("knobs", [PAIR, {}], ids=["pair", "default"])
def test_sigma_zero_pairs(knobs, monkeypatch):
    """the driver's test-episode route: pairs at mutation power 0 are episodes of theta itself"""
    O = _O()
    L = O.layout(O.KIND_GA_LARGE, NACT)
    seeds = np.array([1, 2, 3, 4, 5, 6], np.uint32)
    e = make_engine(monkeypatch, knobs)
    try:
        ret, sg, ln = e.es_eval(np.zeros(3, np.int64), 0.0, TSLIMIT, seeds)
        for m in range(6):
            assert (ret[m // 2, m % 2], sg[m // 2, m % 2], ln[m // 2, m % 2]) == O.rollout(L, theta(), None, seeds[m], TSLIMIT)[:3], m
        assert e.check_redzones() == 0
    finally:
        e.close()


def test_one_pair_short_limits_and_too_many_pairs(monkeypatch):
    from dne_hip import _lib
    O = _O()
    L = O.layout(O.KIND_GA_LARGE, NACT)
    e = make_engine(monkeypatch, PAIR, max_members=4)
    try:
        for T in (1, 2):
            ret, sg, ln = e.es_eval(IDX[:1], SIGMA, T, SEEDS[:2])
            for s in range(2):
                assert (ret[0, s], sg[0, s], ln[0, s]) == O.rollout(L, member_theta(IDX[0], 1 if s == 0 else -1), None, SEEDS[s], T)[:3], (T, s)
        with pytest.raises(_lib.DneError, match="max_members"):
            e.es_eval(IDX[:3], SIGMA, 2, SEEDS[:6])
        assert e.check_redzones() == 0
    finally:
        e.close()


def test_update_and_records(monkeypatch):
    from oracle_engine import OracleEngine
    oret, osg, oln = oracle_eval()
    e = make_engine(monkeypatch, PAIR)
    try:
        ret, sg, ln = e.es_eval(IDX, SIGMA, TSLIMIT, SEEDS)
        assert np.array_equal(ret, oret) and np.array_equal(sg, osg) and np.array_equal(ln, oln)
        for rec in (e.records_pack(5), e.allgather_results(5, 5)):
            assert np.array_equal(rec["noise_idx"], IDX) and np.array_equal(rec["ret"], ret) and np.array_equal(rec["len"], ln)
            assert np.array_equal(rec["aux"], sg)
        e.optimizer_reset()
        e.es_update(IDX, ret, sg, "centered_rank", "adam", 0.005, 0.01)
        oe = OracleEngine(S.KIND_GA_LARGE, NACT)
        oe.noise_upload(S.big_noise())
        oe.set_theta(theta())
        oe.es_update(IDX, oret, osg, "centered_rank", "adam", 0.005, 0.01)
        assert np.array_equal(e.get_theta(), oe.get_theta()) and not np.array_equal(e.get_theta(), theta())
        m, v, t = e.optimizer_get_state()
        om, ov, ot = oe.optimizer_get_state()
        assert t == ot == 1 and np.array_equal(m, om) and np.array_equal(v, ov)
    finally:
        e.close()


def test_driver_equals_the_oracle_engine(monkeypatch, tmp_path):
    """es_gpu.main with exp['model'] = 'LargeModel' on the HIP engine against the same driver on the oracle behind the same method surface"""
    from oracle_engine import OracleEngine
    from dne_hip import _lib, es, es_gpu
    noise = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    noise.noise = S.big_noise()
    noise._engines = []
    exp = {"game": "frostbite", "model": "LargeModel", "num_test_episodes": 2, "population_size": 6, "timesteps": 10 ** 9,
           "episode_cutoff_mode": 20, "return_proc_mode": "centered_rank", "l2coeff": 0.005, "mutation_power": 0.02,
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}}
    e = _lib.Engine(_lib.KIND_GA_LARGE, NACT, max_members=6)
    try:
        sg = es_gpu.main(str(tmp_path / "gpu"), engine=e, noise=noise, seed=2, max_iters=2, **exp)
        assert e.check_redzones() == 0
    finally:
        e.close()
    oe = OracleEngine(S.KIND_GA_LARGE, NACT, max_members=6)
    oe.ref = np.zeros((1, 84, 84, 4), np.uint8)      # the oracle's es_eval wrapper wants an array; the kind ignores it
    noise._engines = []
    so = es_gpu.main(str(tmp_path / "cpu"), engine=oe, noise=noise, seed=2, max_iters=2, **exp)
    assert sg.model == so.model == "LargeModel" and sg.it == so.it == 2 and sg.num_frames == so.num_frames
    assert sg.timesteps_so_far == so.timesteps_so_far > 0
    assert np.array_equal(sg.theta, so.theta)
    assert sg.optimizer[2] == so.optimizer[2] == 2 and np.array_equal(sg.optimizer[0], so.optimizer[0]) and np.array_equal(sg.optimizer[1], so.optimizer[1])


def test_es_and_deep_ga_alternate_on_one_engine(monkeypatch):
    """an ES evaluation, a Deep-GA generation (parents in base slots above 0, children written out), an ES evaluation again: each equals the oracle"""
    O = _O()
    L = O.layout(O.KIND_GA_LARGE, NACT)
    oret, osg, oln = oracle_eval()
    genomes = [(1234,), (200_000, (7, 0.002)), (2_900_000, (5, 0.004), (123_456, 0.001)), (200_000, (7, 0.002), (31_337, 0.003)),
               (4_500_000,), (200_000, (7, 0.002), (31_338, 0.003))]
    gseeds = np.array([21, 22, 23, 24, 25, 26], np.uint32)
    e = make_engine(monkeypatch, PAIR, max_members=16)
    try:
        for _ in range(2):
            ret, sg, ln = e.es_eval(IDX, SIGMA, TSLIMIT, SEEDS)
            assert np.array_equal(ln, oln) and np.array_equal(ret, oret) and np.array_equal(sg, osg)
            assert e.profile()["fc_full_kind"] == 6
            gr, gs, gl = e.ga_eval_powers(genomes, 45, gseeds)
            for i, g in enumerate(genomes):
                assert (gr[i], gs[i], gl[i]) == O.rollout(L, O.ga_gpu_rebuild(S.big_noise(), g, scale_by()), None, gseeds[i], 45)[:3], i
            assert np.array_equal(e.get_theta(), theta())
        assert e.check_redzones() == 0
    finally:
        e.close()
