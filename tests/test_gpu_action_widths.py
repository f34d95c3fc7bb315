"""GPU: every kernel regime at action-set widths other than 18.

The policies take env.action_space.n from the game (gym's minimal action sets have 3..18 actions) and the engine accepts 2..18, but the rest
of the GPU suite runs at 18 (two tests at 14): both even, both with P = 2 (mod 4).  The output layer is the LAST tensor of the flat vector,
[256][A] weights + A biases (LargeModel [512][A]), so the width moves P (P mod 4 = A mod 4 for every small kind: odd P, P = 0 mod 4), makes
the output rows `base + L.ow + tid * A` only 4-byte aligned when A is odd, and sets the candidate count of the speculative tail and of
k_tail_step's fifth wave.  Everything here is bit-exact against the CPU oracle built from oracle/: no tolerances.

Section 1 (every accepted width, 2..18, per engine kind): layout, forward pass (logits, actions, y1..y3 / y1..y4, BN), the ES flat-vector
operations (materialize, theta round trip, Adam / SGD updates) and the GA rebuild (k_chain_sum, k_normc over [256][A]).
Section 2 (widths 3, 4, 9, 17): the lock-step regimes of tests/test_gpu_step_taps.py through that file's own helpers, on engines that record
every member's RAM trajectory: RAM byte 38 is the action of every step, so the argmax of every lock-step of every regime is pinned, and
tests/test_step_tap_cpu.py shows that at 3, 4 and 9 actions the tapped episodes take every action of the set (each candidate lane of the
speculative paths is adopted at least once).

  width 3   smallest real Atari set, P = 3 (mod 4), output rows 12 bytes apart
  width 4   P = 0 (mod 4)
  width 9   odd, more than one 8-wide chunk, P = 1 (mod 4)
  width 17  the largest odd width, one short of the common case"""
import numpy as np
import pytest

import step_tap_support as S
from step_tap_support import NREF, KIND_ES, KIND_GA, KIND_GA_LARGE, KIND_ES_VBN
from test_gpu_edges import _GA_STEP_KNOBS, _VARIANT_KEYS
from test_gpu_step_taps import (ES_REGIMES, _same, _run_es_regime, _run_es_width, _run_ga_regime, _run_large)

pytestmark = pytest.mark.gpu

ALL_WIDTHS = tuple(range(2, 19))
LARGE_WIDTHS = (3, 4, 9, 17)
TAP_WIDTHS = (3, 4, 9, 17)
SHORT_WIDTHS = (3, 9)
SCALES = np.array([0.02, -0.02, 0.0], np.float32)


def _offsets(P, N):
    """slice 0, an odd index, the last legal slice"""
    return np.array([0, 1_000_001, N - P], np.int64)


def _observations(nact):
    obs = np.random.RandomState(100 + nact).randint(0, 256, (3, 84, 84, 4)).astype(np.uint8)
    obs[2, :, :, 1:] = obs[2, :, :, :1]          # (one frame repeated over the stack, as after a reset)
    return obs


def _member(th, noise, off, scale):
    """theta + fl(scale * noise[off : off + P]): two float32 roundings, as every kernel forms a member's weight"""
    return (th + (np.float32(scale) * noise[off:off + th.size]).astype(np.float32)).astype(np.float32)


# ---- section 1: forward pass and flat-vector operations at every accepted width -----------------------------------------------------------
def _check_flat_vector(e, O, kind, nact, th, noise):
    """materialize, theta round trip, three Adam and three SGD updates: the tails of k_materialize, set / get_theta and k_adam's last partial
    block at this P, rows of the materialised output starting at odd float offsets when P is odd"""
    P = e.P
    idx = np.array([1_000_001, noise.size - P], np.int64)
    out = e.materialize(idx, 0.02)
    assert out.shape == (2, 2, P)
    for i, ix in enumerate(idx):
        _same(out[i, 0], O.perturb(th, noise, ix, 0.02, +1), kind, nact, "materialize +", int(ix))
        _same(out[i, 1], O.perturb(th, noise, ix, 0.02, -1), kind, nact, "materialize -", int(ix))
    other = np.random.RandomState(nact).randn(P).astype(np.float32)
    e.set_theta(other)
    _same(e.get_theta(), other, kind, nact, "theta round trip")
    n = 5
    uidx = np.array([0, 3, 1_000_001, 2_222_222, noise.size - P], np.int64)
    for opt, mk in (("adam", lambda: O.Adam(th, 0.01)), ("sgd", lambda: O.SGD(th, 0.01, 0.9))):
        e.set_theta(th); e.optimizer_reset()
        oo = mk()
        for it in range(3):
            rets = (10 * np.random.RandomState(5 + it).poisson(20, (n, 2))).astype(np.float32)
            ratio = e.es_update(uidx, rets, None, "centered_rank", opt, 0.005, 0.01)
            oratio, oth = oo.update(O.es_gradient(noise, uidx, rets, P), 0.005)
            _same(e.get_theta(), oth, kind, nact, opt, it)
            assert abs(ratio - oratio) <= 1e-9 * oratio, (kind, nact, opt, it, ratio, oratio)     # as tests/test_gpu_parity.py::test_reduce_and_update
    e.set_theta(th); e.optimizer_reset()


@pytest.mark.parametrize("nact", ALL_WIDTHS)
@pytest.mark.parametrize("kind", [KIND_ES, KIND_ES_VBN], ids=["es", "vbn"])
def test_es_kinds_forward_and_flat_vector(kind, nact, oracle):
    """ESAtariPolicy and ModelVirtualBN at every width: num_params; three members (+0.02, -0.02, 0 at slice 0, an odd index and the last
    legal slice) through reference pass and dne_act -- BN, y1 / y2 / y3, logits [3][A] and actions equal the oracle's; then the flat-vector
    operations; no kernel wrote outside its buffer"""
    from dne_hip import _lib
    from vbn_support import expand
    O = oracle
    noise = S.small_noise()
    L = O.layout(O.KIND_ES, nact)
    P = S.num_params(kind, nact)
    e = _lib.Engine(kind, nact, max_members=8, ref_count=NREF)
    try:
        assert e.P == P == _lib.num_params(kind, nact) and (kind != KIND_ES or P == L.P)
        e.noise_upload(noise)
        th, ref = S.base_theta(kind, nact), S.ref_batch(nact)
        e.set_theta(th); e.set_ref_batch(ref)
        off, obs = _offsets(P, noise.size), _observations(nact)
        e.set_members(np.zeros(3, np.int32), off, SCALES)
        e.env_set_observation(obs)
        e.ref_pass(3)
        bn = e.get_bn(3)
        acts, logits = e.act(3)
        assert logits.shape == (3, nact) and acts.shape == (3,)
        for i in range(3):
            thi = _member(th, noise, off[i], SCALES[i])
            if kind == KIND_ES_VBN:
                thi = expand(thi, nact)
            obn = O.es_ref_pass(L, thi, ref)
            _same(bn[i], obn, kind, nact, i, "bn")
            y1, y2, y3, lg = O.forward_debug(L, thi, obn, obs[i])
            for name, got, want in zip(("y1", "y2", "y3"), e.debug_activations(i), (y1, y2, y3)):
                _same(got, want, kind, nact, i, name)
            _same(logits[i], lg, kind, nact, i, "logits")
            assert acts[i] == O.act(L, thi, obn, obs[i])[0] == S.argmax_first(lg) and 0 <= acts[i] < nact, (kind, nact, i)
        _check_flat_vector(e, O, kind, nact, th, noise)
        assert e.check_redzones() == 0
    finally:
        e.close()


@pytest.mark.parametrize("mode", ["sign", "centered_sign_rank"])
@pytest.mark.parametrize("kind", [KIND_ES, KIND_ES_VBN], ids=["es", "vbn"])
def test_sign_modes_at_three_actions(kind, mode, oracle):
    """one es_update in the return_proc_modes that use the sign-returns (es.py:283-289), at 3 actions (odd P), against the oracle behind the
    engine surface (tests/oracle_engine.py)"""
    from dne_hip import _lib
    from oracle_engine import OracleEngine
    from vbn_support import OracleVBNEngine
    nact, n = 3, 5
    noise = S.small_noise()
    th = S.base_theta(kind, nact)
    idx = np.array([0, 3, 1_000_001, 2_222_222, noise.size - th.size], np.int64)
    rs = np.random.RandomState(9)
    rets = (10 * rs.poisson(20, (n, 2))).astype(np.float32)
    signs = rs.randint(-6, 7, (n, 2)).astype(np.float32)           # sums of per-step reward signs; ties on purpose
    o = OracleEngine(oracle.KIND_ES, n_actions=nact) if kind == KIND_ES else OracleVBNEngine(n_actions=nact)
    o.noise_upload(noise); o.set_theta(th)
    oratio = o.es_update(idx, rets, signs, mode, "adam", 0.005, 0.01)
    e = _lib.Engine(kind, nact, max_members=8, ref_count=NREF)
    try:
        e.noise_upload(noise); e.set_theta(th)
        ratio = e.es_update(idx, rets, signs, mode, "adam", 0.005, 0.01)
        _same(e.get_theta(), o.get_theta(), kind, mode)
        assert not np.array_equal(o.get_theta(), th) and abs(ratio - oratio) <= 1e-9 * oratio, (kind, mode, ratio, oratio)
        assert e.check_redzones() == 0
    finally:
        e.close()



@pytest.mark.parametrize("nact", ALL_WIDTHS)
def test_ga_rebuild_and_forward(nact, oracle):
    """GAAtariPolicy at every width: ga_rebuild of chains of 1, 2 and 9 seeds (9: the root + one full eight-seed block of k_chain_sum; the root
    goes through k_normc over the [256][A] output tensor) against oracle.ga_rebuild, then three children of those parents through dne_act"""
    from dne_hip import _lib
    O = oracle
    noise = S.small_noise()
    L = O.layout(O.KIND_GA, nact)
    P = S.num_params(KIND_GA, nact)
    hi = noise.size - P
    chains = [[hi], [1_000_001, 0], [4, hi, 3, 1_000_000 + P, 64, 127, 2_222_222, 1, hi - 1]]
    e = _lib.Engine(KIND_GA, nact, max_members=8)
    try:
        assert e.P == P == L.P == _lib.num_params(KIND_GA, nact)
        e.noise_upload(noise)
        parents = []
        for slot, chain in enumerate(chains, 1):
            want = O.ga_rebuild(L, noise, chain, S.GA_SIGMA)
            _same(e.ga_rebuild(slot, chain, S.GA_SIGMA), want, nact, "ga_rebuild", len(chain))
            parents.append(want)
        off, obs = _offsets(P, noise.size), _observations(nact)
        e.set_members(np.array([1, 2, 3], np.int32), off, SCALES)
        e.env_set_observation(obs)
        acts, logits = e.act(3)
        assert logits.shape == (3, nact)
        for i in range(3):
            thi = _member(parents[i], noise, off[i], SCALES[i])
            y1, y2, y3, lg = O.forward_debug(L, thi, None, obs[i])
            for name, got, want in zip(("y1", "y2", "y3"), e.debug_activations(i), (y1, y2, y3)):
                _same(got, want, nact, i, name)
            _same(logits[i], lg, nact, i, "logits")
            assert acts[i] == O.act(L, thi, None, obs[i])[0] == S.argmax_first(lg), (nact, i)
        assert e.check_redzones() == 0
    finally:
        e.close()


@pytest.mark.parametrize("nact", LARGE_WIDTHS)
def test_large_model_rebuild_and_forward(nact, oracle):
    """LargeModel (k_lout over [512][A]): genomes of 1, 2 and 9 seeds rebuilt with ga_rebuild_powers against oracle.ga_gpu_rebuild, then three
    children through dne_act: y1..y4, logits [3][A], actions"""
    from dne_hip import _lib, ga_gpu
    O = oracle
    noise = S.big_noise()
    L = O.layout(O.KIND_GA_LARGE, nact)
    P = S.num_params(KIND_GA_LARGE, nact)
    hi = noise.size - P
    sb = ga_gpu.model_scale_by(nact, KIND_GA_LARGE)
    genomes = [(hi,), (1_234_567, (0, 0.004)),
               (4, (hi, 0.002), (3, 0.004), (2_000_000, 0.001), (64, 0.002), (127, 0.003), (2_222_223, 0.002), (1, 0.004), (hi - 1, 0.002))]
    e = _lib.Engine(KIND_GA_LARGE, nact, max_members=8)
    try:
        assert e.P == P == L.P == sb.size
        e.noise_upload(noise)
        e.ga_set_init_scale(sb)
        parents = []
        for slot, g in enumerate(genomes, 1):
            want = O.ga_gpu_rebuild(noise, g, sb)
            _same(e.ga_rebuild_powers(slot, g), want, nact, "ga_rebuild_powers", len(g))
            parents.append(want)
        off = np.array([0, 1_000_001, hi], np.int64)
        scales = np.array([0.004, 0.002, 0.0], np.float32)
        obs = _observations(nact)
        e.set_members(np.array([1, 2, 3], np.int32), off, scales)
        e.env_set_observation(obs)
        acts, logits = e.act(3)
        assert logits.shape == (3, nact)
        for i in range(3):
            thi = parents[i] if scales[i] == 0 else (parents[i] + scales[i] * noise[off[i]:off[i] + P]).astype(np.float32)   # base.py:141-142
            want = O.forward_large_debug(L, thi, obs[i])
            for name, got, w in zip(("y1", "y2", "y3", "y4"), e.debug_activations_large(i), want[:4]):
                _same(got, w, nact, i, name)
            _same(logits[i], want[4], nact, i, "logits")
            assert acts[i] == S.argmax_first(want[4]), (nact, i)
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- section 2: every lock-step regime at widths 3, 4, 9 and 17 ---------------------------------------------------------------------------
# each regime has its own policy head: k_out<2> (ring, duo), k_out<2, SUB> (sub_out), k_tail_step with its in-launch candidates (sub, the
# tail_fc_* rows, tail_default at 11 pairs) or k_tail_select[_conv1] on the candidates of k_conv1_spec / k_conv2_spec / k_fc_quad_spec
ES_WIDTH_REGIMES = ("ring_product", "ring_product_burst4", "ring_unscaled", "duo", "sub", "sub_out", "tail_default", "tail_spec",
                    "tail_spec_burst4", "tail_fc_quad", "tail_fc_tail", "tail_fc_cols")
VBN_WIDTH_REGIMES = ("ring_product", "tail_default", "tail_spec", "tail_fc_cols")
assert set(ES_WIDTH_REGIMES) | set(VBN_WIDTH_REGIMES) <= set(ES_REGIMES)


@pytest.mark.parametrize("nact", TAP_WIDTHS)
@pytest.mark.parametrize("name", ES_WIDTH_REGIMES)
def test_es_regime_taps_at_width(name, nact, monkeypatch):
    """the 11 edge-index pairs of that width's P at sigma 0.02, T = 1, 3, 9: y2 / y3 rows, BN, returns, lengths == T, fc_full_kind where
    the regime has one, and all 22 RAM trajectories [T][128]"""
    _run_es_regime(KIND_ES, name, monkeypatch, nact, sigmas=(0.02,), check_ram=True)


@pytest.mark.parametrize("nact", TAP_WIDTHS)
@pytest.mark.parametrize("pairs", [2, 5])
@pytest.mark.parametrize("name", ["ring_product", "tail_default"])
def test_es_pair_counts_at_width(name, pairs, nact, monkeypatch):
    """2 pairs: one full ring workgroup, and by default the speculative tail (k_conv1_spec, k_conv2_spec, k_fc_quad_spec,
    k_tail_select[_conv1]: A candidates per member); 5 pairs: a partial last ring workgroup, one window falling to the tail kernels"""
    _run_es_width(pairs, name, monkeypatch, nact, check_ram=True)


@pytest.mark.parametrize("nact", SHORT_WIDTHS)
@pytest.mark.parametrize("name", VBN_WIDTH_REGIMES)
def test_vbn_regime_taps_at_width(name, nact, monkeypatch):
    """ModelVirtualBN (the heads' no-bias paths; its out/b is still there) on its own P of that width"""
    _run_es_regime(KIND_ES_VBN, name, monkeypatch, nact, sigmas=(0.02,), check_ram=True)


def _ga_width_params():
    out = [pytest.param({}, id="default")]                     # both member orders (DNE_GA_SORT)
    for k in _GA_STEP_KNOBS:
        if not _VARIANT_KEYS & set(k):
            out.append(pytest.param(k, id=",".join("%s=%s" % kv for kv in k.items())))
    return out


@pytest.mark.parametrize("nact", SHORT_WIDTHS)
@pytest.mark.parametrize("knobs", _ga_width_params())
def test_ga_regime_taps_at_width(knobs, nact, monkeypatch):
    """test_ga_regime_taps at 3 and 9 actions: roots and mutation seeds on the edge set of that width's P; y2 / y3 and the final RAM"""
    _run_ga_regime(knobs, monkeypatch, nact)


@pytest.mark.parametrize("nact", SHORT_WIDTHS)
@pytest.mark.parametrize("knobs", [pytest.param({}, id="6-default"), pytest.param({"DNE_GA_MATERIALIZE": "0"}, id="6-on_the_fly")])
def test_large_model_taps_at_width(knobs, nact, oracle, monkeypatch):
    """test_large_model_taps' six-member cases (children written out / parent + noise rows on the fly) at 3 and 9 actions: y1..y4"""
    _run_large(6, knobs, monkeypatch, nact)
