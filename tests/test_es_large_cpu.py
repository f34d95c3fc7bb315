"""CPU: what ES over the GPU tree's LargeModel adds outside the kernels -- the planner's pair regime (csrc/plan.h: k_lfc_pair for antithetic pairs over
base slot 0 in windows above lfc_cols_max MEMBERS, every LargeModel threshold counted in members) and the es_gpu.py driver with
exp['model'] = 'LargeModel' on the oracle behind the Engine surface."""
import pickle

import numpy as np
import pytest

import step_tap_support as S

KIND_LARGE, NACT = 2, 18
PAIRS = dict(antithetic_slot0=1, uniform_base=1)


def _plan(total, gsize, **facts):
    from dne_hip import _lib
    return [(r.cnt, _lib.FC_NAMES[r.fc], r.s1, r.s2, r.conv) for r in _lib.debug_plan(KIND_LARGE, NACT, total, gsize, **facts)]


def test_fc_names_keep_their_numbers():
    from dne_hip import _lib
    assert _lib.FC_NAMES[:10] == ("k_lfc_cols", "k_lfc", "k_fc_sub", "k_fc_quad", "k_fc_tail", "k_fc_cols", "k_fc_ring", "k_fc_duo", "k_fc2", "k_fc")
    assert _lib.FC_NAMES[10:] == ("k_lfc_pair",)


def test_pairs_plan_by_members(monkeypatch):
    from dne_hip import _lib
    for k in ("DNE_NSUB", "DNE_LFC_COLS_MAX", "DNE_FC_TAIL_MAX"):
        monkeypatch.delenv(k, raising=False)
    seen = set()
    for total in list(range(1, 120)) + [192, 193, 256, 257, 300, 384, 385, 400, 512, 513, 799, 800, 1000, 1899, 1900, 2500]:
        rows = _plan(total, 2, **PAIRS)
        assert sum(r[0] for r in rows) == total
        for cnt, fc, s1, s2, conv in rows:
            members = 2 * cnt
            assert fc == ("k_lfc_cols" if cnt <= 48 else "k_lfc_pair"), (total, cnt)        # 48 pairs = 96 members = lfc_cols_max
            assert s1 == s2 == (4 if members <= 128 else 2 if members <= 256 else 1), (total, cnt)
            assert conv == 0
            seen.add((fc, s2))
        widest = max(r[0] for r in rows)
        assert _lib.debug_plan(KIND_LARGE, NACT, total, 2, whole_eval=True, **PAIRS) == (6 if widest > 48 else 1), total
    assert seen == {("k_lfc_cols", 4), ("k_lfc_pair", 4), ("k_lfc_pair", 2), ("k_lfc_pair", 1)}
    # one window: the threshold itself
    monkeypatch.setenv("DNE_NSUB", "1")
    assert [r[:2] for r in _plan(48, 2, **PAIRS)] == [(48, "k_lfc_cols")] and [r[:2] for r in _plan(49, 2, **PAIRS)] == [(49, "k_lfc_pair")]
    assert [r[3] for r in _plan(64, 2, **PAIRS)] == [4] and [r[3] for r in _plan(65, 2, **PAIRS)] == [2]
    assert [r[3] for r in _plan(128, 2, **PAIRS)] == [2] and [r[3] for r in _plan(129, 2, **PAIRS)] == [1]
    monkeypatch.setenv("DNE_LFC_COLS_MAX", "0")
    assert [r[:2] for r in _plan(1, 2, **PAIRS)] == [(1, "k_lfc_pair")]
    assert _lib.debug_plan(KIND_LARGE, NACT, 1, 2, whole_eval=True, **PAIRS) == 6


def test_pairs_without_antithetic_slot0_stay_on_the_member_kernels(monkeypatch):
    from dne_hip import _lib
    monkeypatch.delenv("DNE_NSUB", raising=False)
    for facts in ({}, dict(uniform_base=1), dict(uniform_base=1, pair_sigma_uniform=1)):
        for total in (1, 48, 96, 98, 100, 300, 1000):
            for cnt, fc, s1, s2, conv in _plan(total, 2, **facts):
                assert fc == ("k_lfc_cols" if cnt <= 48 else "k_lfc"), (facts, total, cnt)
            assert _lib.debug_plan(KIND_LARGE, NACT, total, 2, whole_eval=True, **facts) == 1


def test_groups_of_one_plan_as_before(monkeypatch):
    from dne_hip import _lib
    monkeypatch.delenv("DNE_NSUB", raising=False)
    for facts in ({}, dict(members_materialized=1), PAIRS):   # (facts a member set of single groups may carry: never the pair kernel)
        for total in list(range(1, 200)) + [256, 257, 384, 385, 512, 513, 1000, 1028, 2000]:
            rows = _lib.debug_plan(KIND_LARGE, NACT, total, 1, **facts)
            for r in rows:
                assert _lib.FC_NAMES[r.fc] == ("k_lfc_cols" if r.cnt <= 96 else "k_lfc"), (total, r.cnt)
                assert r.s1 == r.s2 == (4 if r.cnt <= 128 else 2 if r.cnt <= 256 else 1)
                assert r.wide == int(r.cnt > 96) and r.conv == 0
            assert _lib.debug_plan(KIND_LARGE, NACT, total, 1, whole_eval=True, **facts) == 1


# ---- the driver on the oracle ------------------------------------------------------------------------------------------------------------
def _exp(**over):
    exp = {"game": "frostbite", "model": "LargeModel", "num_test_episodes": 1, "population_size": 4, "timesteps": 10 ** 9,
           "episode_cutoff_mode": 10, "return_proc_mode": "centered_rank", "l2coeff": 0.005, "mutation_power": 0.02,
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}}
    exp.update(over)
    return exp


def _noise():
    from dne_hip import es
    noise = es.SharedNoiseTable.__new__(es.SharedNoiseTable)
    noise.noise = S.big_noise()
    noise._engines = []
    return noise


def _large_engine():
    from oracle_engine import OracleEngine
    e = OracleEngine(KIND_LARGE, NACT, max_members=4)
    e.ref = np.zeros((1, 84, 84, 4), np.uint8)     # the oracle's es_eval wrapper wants an array; the kind ignores it
    return e


def test_driver_start_point_resume_and_refusals(oracle, tmp_path):
    from oracle_engine import OracleEngine
    from dne_hip import _lib, es_gpu, ga_gpu
    noise = _noise()

    def run(log_dir, iters, eng=None, **over):
        eng = eng or _large_engine()
        return es_gpu.main(str(log_dir), engine=eng, noise=noise, seed=4, max_iters=iters, **_exp(**over)), eng

    st0, e0 = run(tmp_path / "zero", 0)
    P = e0.P
    assert P == 4052658 and st0.model == "LargeModel" and st0.num_params == P and st0.it == 0 and e0.ref.shape[0] == 1
    idx = np.random.RandomState(4).randint(0, noise.noise.size - P + 1)          # the first draw of the run's stream
    th0 = noise.get(idx, P) * ga_gpu.model_scale_by(NACT, _lib.KIND_GA_LARGE)
    assert th0.dtype == np.float32 and np.array_equal(st0.theta, th0)
    assert np.array_equal(e0.scale_by, ga_gpu.model_scale_by(NACT, _lib.KIND_GA_LARGE))

    st1, _ = run(tmp_path / "one", 1)
    st2, _ = run(tmp_path / "two", 2)
    assert st2.it == 2 and st2.optimizer[2] == 2 and not np.array_equal(st2.theta, th0) and st2.timesteps_so_far > 0
    st1b, _ = run(tmp_path / "one", 1)                                           # resumes from the one-iteration run's snapshot.pkl
    assert st1b.it == 2 and st1b.timesteps_so_far == st2.timesteps_so_far and np.array_equal(st1b.theta, st2.theta)
    for a, b in zip(st1b.optimizer[:2], st2.optimizer[:2]):
        assert np.array_equal(a, b)
    snap = pickle.load(open(tmp_path / "two" / "snapshot.pkl", "rb"))
    assert snap.model == "LargeModel" and snap.flat_layout == "native" and snap.num_params == P

    with pytest.raises(ValueError, match=r"'LargeModel'.*4052658.*'ModelVirtualBN'.*1009058"):
        run(tmp_path / "two", 1, eng=OracleEngine(0, ref_count=8, max_members=4), model="ModelVirtualBN")
    # the engine passed in selects the path; a config that names another model or layout is refused
    with pytest.raises(ValueError, match="ModelVirtualBN"):
        run(tmp_path / "other", 1, model="ModelVirtualBN")
    with pytest.raises(ValueError, match="flat_layout"):
        run(tmp_path / "other", 1, flat_layout="es_distributed")
    st, _ = run(tmp_path / "native", 0, flat_layout="native")
    assert st.flat_layout == "native"


def test_driver_refuses_other_models_and_momentum_one(tmp_path):
    from dne_hip import es_gpu
    for name in ("Model", "ModelBN", "SmallDQN", "NoSuchModel"):
        with pytest.raises(NotImplementedError, match=name):
            es_gpu.main(str(tmp_path / name), noise=_noise(), seed=0, max_iters=1, **_exp(model=name))
        with pytest.raises(NotImplementedError, match=name):
            es_gpu.main(str(tmp_path / name), engine=_large_engine(), noise=_noise(), seed=0, max_iters=1, **_exp(model=name))
    with pytest.raises(ValueError, match="momentum"):
        es_gpu.engine_optimizer({"type": "sgd", "args": {"stepsize": 0.01, "momentum": 1.0}})
    assert es_gpu.engine_optimizer({"type": "sgd", "args": {"stepsize": 0.01, "momentum": 0.5}})[1] == 0.02
    with pytest.raises(ValueError, match="momentum"):
        es_gpu.main(str(tmp_path / "sgd"), engine=_large_engine(), noise=_noise(), seed=0, max_iters=1,
                    **_exp(optimizer={"type": "sgd", "args": {"stepsize": 0.01, "momentum": 1}}))
