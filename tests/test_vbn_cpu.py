"""ModelVirtualBN's own flat layout (DNE_KIND_ES_VBN) on the host: the layout, scale_by, the map onto the ES kind's vector, and the GPU
tree's ES driver with exp['flat_layout'] = 'native' on the CPU oracle (tests/vbn_support.py)."""
import pickle

import numpy as np
import pytest

from vbn_support import KIND_ES_VBN, OracleVBNEngine, contract, expand

LAYOUT = [("layer1/conv1/w", (8, 8, 4, 16), 0), ("layer1/BatchNorm/b", (1, 1, 1, 16), 4096),
          ("layer2/conv2/w", (4, 4, 16, 32), 4112), ("layer2/BatchNorm/b", (1, 1, 1, 32), 12304),
          ("layer3/fc/w", (3872, 256), 12336), ("layer3/BatchNorm/b", (1, 256), 1003568),
          ("layer4/out/w", (256, "A"), 1003824), ("layer4/out/b", (1, "A"), None)]


@pytest.mark.parametrize("nact, P", [(18, 1008450), (14, 1007422)])
def test_flat_layout_names_offsets_and_size(nact, P):
    from dne_hip import _lib, policies
    assert _lib.KIND_ES_VBN == KIND_ES_VBN and KIND_ES_VBN in _lib.ES_KINDS
    spec, n = policies.flat_layout(_lib.KIND_ES_VBN, nact)
    assert n == P == 1003824 + 257 * nact
    assert list(spec) == [name for name, _, _ in LAYOUT]
    for name, shape, off in LAYOUT:
        shape = tuple(nact if s == "A" else s for s in shape)
        off = 1003824 + 256 * nact if off is None else off
        assert spec[name] == (off, shape), name
    last_off, last_shape = spec["layer4/out/b"]
    assert last_off + int(np.prod(last_shape)) == P


def test_num_params_from_the_library():
    from dne_hip import _lib
    lib = _lib.load()
    assert lib.dne_num_params(_lib.KIND_ES_VBN, 18) == 1008450 and lib.dne_num_params(_lib.KIND_ES_VBN, 14) == 1007422
    assert lib.dne_num_params(_lib.KIND_ES, 18) == 1009058   # the ES kind did not move


def test_scale_by():
    from dne_hip import _lib, policies
    sb = policies.vbn_scale_by(18)
    spec, P = policies.flat_layout(_lib.KIND_ES_VBN, 18)
    assert sb.dtype == np.float32 and sb.shape == (P,)
    want = {"layer1/conv1/w": 1 / 16, "layer2/conv2/w": 1 / 16, "layer3/fc/w": 1 / np.sqrt(3872), "layer4/out/w": 1 / 16}
    for name, (off, shape) in spec.items():
        seg = sb[off:off + int(np.prod(shape))]
        assert np.all(seg == np.float32(want.get(name, 0.0))), name   # std 1.0 for out/w too (batchnorm.py:105); every b 0


@pytest.mark.parametrize("nact", [18, 14])
def test_expand_round_trip(nact):
    from dne_hip import _lib, policies
    espec, Pes = policies.flat_layout(_lib.KIND_ES, nact)
    th = np.random.RandomState(nact).randn(1003824 + 257 * nact).astype(np.float32)
    ex = expand(th, nact)
    assert ex.shape == (Pes,) and np.array_equal(contract(ex, nact), th)
    for name in ("conv1/biases", "conv2/biases", "fc/biases"):
        off, shape = espec[name]
        seg = ex[off:off + int(np.prod(shape))]
        assert np.all(seg == 0.0) and not np.signbit(seg).any(), name   # +0.0f exactly
    for name in ("BatchNorm/gamma", "BatchNorm_1/gamma", "BatchNorm_2/gamma"):
        off, shape = espec[name]
        assert np.all(ex[off:off + int(np.prod(shape))] == 1.0), name
    off, _ = espec["BatchNorm_2/beta"]
    assert np.array_equal(ex[off:off + 256], th[1003568:1003824])


def _exp(**over):
    exp = {"game": "frostbite", "model": "ModelVirtualBN", "num_test_episodes": 2, "population_size": 6, "timesteps": 10 ** 9,
           "episode_cutoff_mode": "adaptive:6,0.3,2,20", "return_proc_mode": "centered_rank", "l2coeff": 0.005,
           "mutation_power": {"type": "LinearSchedule", "schedule": 4, "initial_p": 0.02, "final_p": 0.01, "field": "iteration"},
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}, "flat_layout": "native"}
    exp.update(over)
    return exp


def test_es_driver_native_layout_start_point_and_resume(oracle, tmp_path):
    """es_gpu.main(flat_layout='native'): theta_0 = noise.get(idx, P) * scale_by with idx the run stream's first draw (es.py:73-75,
    base.py:123-141); one iteration + a resumed one equal two uninterrupted iterations; a resume across layouts fails and names both."""
    from oracle_engine import OracleEngine
    from dne_hip import es, es_gpu, policies
    noise = es.SharedNoiseTable(count=2_500_000)
    exp = _exp()

    def run(log_dir, iters, eng=None, **over):
        eng = eng or OracleVBNEngine(ref_count=8, max_members=6)
        return es_gpu.main(str(log_dir), engine=eng, noise=noise, seed=4, max_iters=iters, **dict(exp, **over)), eng

    st0, e0 = run(tmp_path / "zero", 0)
    P = e0.P
    assert P == 1008450 and st0.flat_layout == "native" and st0.num_params == P and st0.it == 0
    idx = np.random.RandomState(4).randint(0, noise.noise.size - P + 1)
    th0 = noise.get(idx, P) * policies.vbn_scale_by(18)
    assert th0.dtype == np.float32 and np.array_equal(st0.theta, th0)

    st1, _ = run(tmp_path / "one", 1)
    st2, _ = run(tmp_path / "two", 2)
    assert st2.it == 2 and st2.optimizer[2] == 2 and st2.theta.size == P and not np.array_equal(st2.theta, th0)
    st1b, _ = run(tmp_path / "one", 1)                              # resumes from snapshot.pkl of the one-iteration run
    assert st1b.it == 2 and st1b.tslimit == st2.tslimit and st1b.timesteps_so_far == st2.timesteps_so_far
    assert np.array_equal(st1b.theta, st2.theta)
    for a, b in zip(st1b.optimizer[:2], st2.optimizer[:2]):
        assert np.array_equal(a, b)
    snap = pickle.load(open(tmp_path / "two" / "snapshot.pkl", "rb"))
    assert snap.flat_layout == "native" and snap.num_params == P

    # a native snapshot resumed by an es_distributed run, and the other way round
    with pytest.raises(ValueError, match=r"'native'.*1008450.*'es_distributed'.*1009058"):
        run(tmp_path / "two", 1, eng=OracleEngine(0, ref_count=8, max_members=6), flat_layout="es_distributed")
    run(tmp_path / "es", 1, eng=OracleEngine(0, ref_count=8, max_members=6), flat_layout="es_distributed")
    with pytest.raises(ValueError, match=r"'es_distributed'.*1009058.*'native'.*1008450"):
        run(tmp_path / "es", 1)
    # a snapshot written before the key existed reads as es_distributed
    old = pickle.load(open(tmp_path / "es" / "snapshot.pkl", "rb"))
    del old.flat_layout, old.num_params
    pickle.dump(old, open(tmp_path / "es" / "snapshot.pkl", "wb"))
    with pytest.raises(ValueError, match=r"'es_distributed'.*'native'"):
        run(tmp_path / "es", 1)
    st, _ = run(tmp_path / "es", 1, eng=OracleEngine(0, ref_count=8, max_members=6), flat_layout="es_distributed")
    assert st.it == 2 and st.flat_layout == "es_distributed"
    # the engine passed in decides; a config that names another layout is refused
    with pytest.raises(ValueError, match="flat_layout"):
        run(tmp_path / "x", 1, eng=OracleEngine(0, ref_count=8, max_members=6))
