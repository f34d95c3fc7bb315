"""The ModelVirtualBN engine kind (DNE_KIND_ES_VBN) on the GPU against the unchanged CPU oracle: every member's vector expanded onto the ES
kind's layout (+0.0f conv / fc biases, 1.0f BN gammas, tests/vbn_support.py) must give the same bits -- BN scale / shift and moments, the
activations, logits, actions, returns, lengths, RAM trajectories -- through every fc kernel of the ES product path, and the update on the
native P must be the oracle's weighted sum + Adam."""
import numpy as np
import pytest

from vbn_support import OracleVBNEngine, es_pairs, expand

pytestmark = pytest.mark.gpu

NREF = 16
NACT = 18
P = 1008450


@pytest.fixture(scope="module")
def hip():
    from dne_hip import _lib
    return _lib


@pytest.fixture(scope="module")
def ref_batch(oracle):
    return oracle.get_ref_batch(seed=0, batch_size=NREF, nact=NACT)


@pytest.fixture(scope="module")
def vbn_engine(hip, small_noise):
    e = hip.Engine(hip.KIND_ES_VBN, NACT, max_members=64, ref_count=NREF, record_bc=True, bc_max_steps=224, profile_events=True)
    e.noise_upload(small_noise)
    yield e
    e.close()


def _theta(noise, at, seed):
    """a ModelVirtualBN start point (noise slice * scale_by, base.py:123-141) moved off it so that every BatchNorm/b is nonzero"""
    from dne_hip import policies
    rs = np.random.RandomState(seed)
    return noise[at:at + P] * policies.vbn_scale_by(NACT) + (0.01 * rs.randn(P)).astype(np.float32)


def test_engine_kind_layout(vbn_engine, hip):
    assert vbn_engine.P == P == hip.num_params(hip.KIND_ES_VBN, NACT)
    assert vbn_engine.ref_count == NREF


def test_forward_bit_exact(vbn_engine, oracle, small_noise, ref_batch):
    e, O = vbn_engine, oracle
    L = O.layout(O.KIND_ES, NACT)
    bases = [_theta(small_noise, 777, 1), _theta(small_noise, 1_234_567, 2)]
    for s, th in enumerate(bases):
        e.set_theta(th, s)
    e.set_ref_batch(ref_batch)
    rs = np.random.RandomState(3)
    n = 10
    off = rs.randint(0, small_noise.size - P, n).astype(np.int64)
    off[1] = off[0]                                             # an antithetic pair
    slot = np.array([0, 0, 1, 1, 0, 1, 0, 1, 1, 0], np.int32)
    scale = np.array([0.02, -0.02, 0.0, 0.5, 0.02, 0.01, -0.05, 0.02, 0.0, 0.003], np.float32)
    e.set_members(slot, off, scale)
    obs = rs.randint(0, 256, (n, 84, 84, 4)).astype(np.uint8)
    obs[4] = ref_batch[2]; obs[5] = 0; obs[6] = 255
    e.env_set_observation(obs)
    e.ref_pass(n)
    bn = e.get_bn(n)
    mom = e.get_bn_moments(n)
    acts, logits = e.act(n)
    for i in range(n):
        thi = expand(bases[slot[i]] + np.float32(scale[i]) * small_noise[off[i]:off[i] + P], NACT)
        obn, omom = O.es_ref_pass_moments(L, thi, ref_batch)
        assert np.array_equal(bn[i], obn), i
        assert np.array_equal(mom[i], omom), i
        y1, y2, y3, lg = O.forward_debug(L, thi, obn, obs[i])
        g1, g2, g3 = e.debug_activations(i)
        assert np.array_equal(g1, y1) and np.array_equal(g2, y2) and np.array_equal(g3, y3), i
        assert np.array_equal(logits[i], lg), i
        assert acts[i] == O.act(L, thi, obn, obs[i])[0], i


# the small evaluation's inputs: 8 pairs, cutoff 125 (four pairs end by game over before it, the others run into it)
N_SMALL, TSL_SMALL, SIGMA = 8, 125, 0.02


@pytest.fixture(scope="module")
def small_eval(oracle, small_noise, ref_batch):
    th = _theta(small_noise, 777, 11)
    srs = np.random.RandomState(0)
    idx = np.array([srs.randint(0, small_noise.size - P + 1) for _ in range(N_SMALL)], np.int64)
    seeds = np.random.RandomState(1000).randint(0, 2 ** 31, 2 * N_SMALL).astype(np.uint32)
    ret, sg, ln, bcs = es_pairs(small_noise, th, ref_batch, idx, seeds, SIGMA, TSL_SMALL, NACT, want_bc=True)
    return dict(th=th, idx=idx, seeds=seeds, ret=ret, sg=sg, ln=ln, bcs=bcs)


def test_es_eval_small_matches_oracle(vbn_engine, small_eval, ref_batch):
    e, o = vbn_engine, small_eval
    e.set_theta(o["th"])
    e.set_ref_batch(ref_batch)
    ret, sg, ln, bc = e.es_eval(o["idx"], SIGMA, TSL_SMALL, o["seeds"], want_bc=True)
    assert np.array_equal(ln, o["ln"]) and np.array_equal(ret, o["ret"]) and np.array_equal(sg, o["sg"])
    assert ln.min() < TSL_SMALL <= ln.max()                     # an early game over and the cutoff
    m = 5                                                       # pair 2, the -sigma member
    assert ln.reshape(-1)[m] == len(o["bcs"][m]) and np.array_equal(bc[m, :len(o["bcs"][m])], o["bcs"][m])
    assert e.profile()["env_steps"] == ln.sum()


# knobs of INTEGRATION.md section 5 that put each fc kernel of the ES product path onto the small population, with the fc_full_kind the
# profile must report (5 = k_fc_ring, 3 = k_fc_duo, 4 = k_fc_sub); None: a tail / convolution schedule, the kind is not the point
KNOBS = [
    ({"DNE_FC_RING": "2", "DNE_FC_DUO_MIN": "2", "DNE_FC_TAIL_MAX": "1"}, 5),                        # k_fc_ring<true> (scaled table copy)
    ({"DNE_FC_RING": "2", "DNE_FC_DUO_MIN": "2", "DNE_FC_TAIL_MAX": "1", "DNE_RING_PRE": "0"}, 5),   # k_fc_ring<false>
    ({"DNE_FC_RING": "1", "DNE_FC_DUO_MIN": "2", "DNE_FC_TAIL_MAX": "1", "DNE_DUO_SOLO_BELOW": "0", "DNE_RING_MIN": "0"}, 5),   # its default gate
    ({"DNE_FC_RING": "2", "DNE_FC_DUO_MIN": "2", "DNE_FC_TAIL_MAX": "1", "DNE_CONV_FUSED_MIN": "1"}, 5),   # behind k_conv12
    ({"DNE_FC_RING": "0", "DNE_FC_DUO_MIN": "2", "DNE_FC_TAIL_MAX": "1"}, 3),                        # k_unit_order + k_fc_duo + k_out
    ({"DNE_FC_SUB": "2", "DNE_FC_SUB_MIN": "2"}, 4),                                                 # k_fc_sub + k_out<.., SUB>
    ({"DNE_SPEC_MAX": "0"}, None),                                                                   # k_tail_step, no speculative tail
    ({"DNE_SPEC_MAX": "0", "DNE_FC_QUAD_MAX": "0", "DNE_FC_TAILK_MAX": "0"}, None),                  # k_fc_cols
    ({"DNE_SPEC_MAX": "0", "DNE_CONV12T_MAX": "0"}, None),                                           # k_conv1 + k_conv2 in the tail
]


@pytest.mark.parametrize("knobs, kind", KNOBS, ids=[",".join("%s=%s" % kv for kv in k.items()) for k, _ in KNOBS])
def test_es_eval_fc_kernels_match_oracle(hip, small_eval, small_noise, ref_batch, monkeypatch, knobs, kind):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    o = small_eval
    e = hip.Engine(hip.KIND_ES_VBN, NACT, max_members=2 * N_SMALL, ref_count=NREF, profile_events=True)
    try:
        e.noise_upload(small_noise)
        e.set_ref_batch(ref_batch)
        e.set_theta(o["th"])
        ret, sg, ln = e.es_eval(o["idx"], SIGMA, TSL_SMALL, o["seeds"])
        assert np.array_equal(ln, o["ln"]) and np.array_equal(ret, o["ret"]) and np.array_equal(sg, o["sg"]), knobs
        if kind is not None:
            assert e.profile()["fc_full_kind"] == kind, knobs
    finally:
        e.close()


@pytest.mark.variants
@pytest.mark.parametrize("knobs", [{"DNE_FC_DUO": "0", "DNE_FC2_MIN": "2", "DNE_FC_TAIL_MAX": "1"},    # k_fc2 (forward_variants.h)
                                   {"DNE_CONV1_SHARED": "0"}])                                          # k_conv1_ref (forward_variants.h)
def test_es_eval_variant_kernels_match_oracle(hip, small_eval, small_noise, ref_batch, monkeypatch, knobs):
    test_es_eval_fc_kernels_match_oracle(hip, small_eval, small_noise, ref_batch, monkeypatch, knobs, None)


def test_es_update_matches_oracle(vbn_engine, oracle, small_noise):
    e, O = vbn_engine, oracle
    n = 96
    srs = np.random.RandomState(0)
    idx = np.array([srs.randint(0, small_noise.size - P + 1) for _ in range(n)], np.int64)
    th0 = _theta(small_noise, 4321, 5)
    e.set_theta(th0); e.optimizer_reset()
    opt = O.Adam(th0, 0.01)
    for it in range(3):
        rets = (10 * np.random.RandomState(5 + it).poisson(20, (n, 2))).astype(np.float32)
        ratio = e.es_update(idx, rets, None, "centered_rank", "adam", 0.005, 0.01)
        proc = O.centered_ranks(rets.reshape(-1)).reshape(n, 2)
        og = O.weighted_sum(small_noise, idx, proc[:, 0] - proc[:, 1], P, float(rets.size))
        oratio, oth = opt.update(og, 0.005)
        assert oth.shape == (P,) and np.array_equal(e.get_theta(), oth), it
        assert abs(ratio - oratio) <= 1e-9 * oratio


def test_gpu_tree_es_driver_native_equals_the_oracle_engine(hip, tmp_path):
    """es_gpu.main(flat_layout='native') on the HIP engine and on the CPU stand-in: two iterations, theta and Adam's state bit for bit"""
    from dne_hip import es, es_gpu
    noise = es.SharedNoiseTable(count=2_500_000)
    exp = {"game": "frostbite", "model": "ModelVirtualBN", "num_test_episodes": 3, "population_size": 8, "timesteps": 10 ** 9,
           "episode_cutoff_mode": "adaptive:10,0.3,2,40", "return_proc_mode": "centered_rank", "l2coeff": 0.005,
           "mutation_power": {"type": "LinearSchedule", "schedule": 4, "initial_p": 0.02, "final_p": 0.01, "field": "iteration"},
           "optimizer": {"args": {"stepsize": 0.01}, "type": "adam"}, "flat_layout": "native"}
    e = hip.Engine(hip.KIND_ES_VBN, NACT, max_members=8, ref_count=NREF)
    try:
        sg = es_gpu.main(str(tmp_path / "gpu"), engine=e, noise=noise, seed=2, max_iters=2, **exp)
    finally:
        e.close()
    so = es_gpu.main(str(tmp_path / "cpu"), engine=OracleVBNEngine(ref_count=NREF, max_members=8), noise=noise, seed=2, max_iters=2, **exp)
    assert sg.flat_layout == so.flat_layout == "native" and sg.theta.size == P
    assert sg.it == so.it == 2 and sg.tslimit == so.tslimit and sg.timesteps_so_far == so.timesteps_so_far and sg.num_frames == so.num_frames
    assert np.array_equal(sg.theta, so.theta)
    assert sg.optimizer[2] == so.optimizer[2] == 2
    assert np.array_equal(sg.optimizer[0], so.optimizer[0]) and np.array_equal(sg.optimizer[1], so.optimizer[1])


def test_full_width_generation_matches_oracle(hip, oracle, noise_table):
    """2 500 pairs on the 250 M table with a short cutoff: the product schedule from the full-width kernels down to the tail; pairs spread
    over the population, the shortest and the longest included, bit-exact against the expanded oracle"""
    from dne_hip import es, policies
    n, sigma, tslimit = 2500, 0.02, 300
    e = hip.Engine(hip.KIND_ES_VBN, NACT, max_members=2 * n, ref_count=128)
    try:
        noise_table.attach(e)
        rs = np.random.RandomState(0)
        th = noise_table.get(noise_table.sample_index(rs, P), P) * policies.vbn_scale_by(NACT)
        ref = oracle.get_ref_batch(seed=0, batch_size=128, nact=NACT)
        e.set_theta(th)
        e.set_ref_batch(ref)
        _, idx, seeds = es.generation_inputs(noise_table.noise.size, P, n, 0, 0, 1)
        ret, sg, ln = e.es_eval(idx, sigma, tslimit, seeds)
    finally:
        e.close()
    tot = ln.sum(axis=1)
    pick = sorted({int(np.argmin(tot)), int(np.argmax(tot))} | set(np.linspace(0, n - 1, 8).astype(int).tolist()))
    assert len(pick) >= 8
    oret, osg, oln, _ = es_pairs(noise_table.noise, th, ref, idx[pick], seeds.reshape(-1, 2)[pick].reshape(-1), sigma, tslimit, NACT)
    assert np.array_equal(ln[pick], oln) and np.array_equal(ret[pick], oret) and np.array_equal(sg[pick], osg)
