"""GPU: the sub-slice fc's dead rows.  k_fc_sub fetches a row of zeros in place of a weight row whose activation relu(bn2(y2)) is +0 in
every member the launch computes: same loads, same window, another base address.  A wrong live mask -- a bit of the
wrong row, of the wrong 64-row half of the chain, of the block behind the one it belongs to -- drops a row that counts, and y3 differs.

Every form of the kernel is forced onto 6 pairs through the rows of test_gpu_edges._ES_STEP_KNOBS whose widest window is k_fc_sub (1 / 2 / 8
chains per wave, one and two windows, both heads behind it) and evaluated on base vectors whose bn2 shift makes liveness exact BY CHANNEL
(row k of the fc matrix meets channel k mod 32): a channel with shift -BIG is dead on every row, with +BIG alive on every row, whatever the
frame -- the test checks that on the oracle's own activations before it compares.  Channels 0 and 31 alone put the live row first / last in
every 8-row block, at the 64-row border inside a chain and at the 128 / 120-row chain borders.  y2, y3, the batch-norm rows, returns and
every step's RAM (byte 38 = the action) are compared with the oracle value by value, as tests/test_gpu_step_taps.py does.  The GA's
k_fc_sub<1, false, false> (no batch norm, one member per group: it skips on that member's own zeros; 1 and 4 chains per wave) and every ES
form also run a short rollout against the oracle."""
import functools

import numpy as np
import pytest

import oracle as O
import step_tap_support as S
from step_tap_support import NACT, NREF, KIND_ES
from test_gpu_edges import _ES_STEP_KNOBS, _GA_STEP_KNOBS, _VARIANT_KEYS

pytestmark = pytest.mark.gpu

SIGMA = 0.02
T = 3                     # lock-steps per crafted case: a burst's first and two more
BIG = np.float32(1000.0)  # |gamma * (y - mean) / std| of a channel stays below sqrt(16 * 121) = 44 on the reference frames; the noise moves a shift by ~0.02
F_CH = 5                  # case (f): the channel whose shift is 0 in theta and +-1 in the two members
CASES = ("all_dead", "all_live", "ch0", "ch31", "even_dead", "split")
_LIVE = {"all_dead": (), "all_live": range(32), "ch0": (0,), "ch31": (31,), "even_dead": range(1, 32, 2), "split": ()}


def _is_sub(k):
    return "DNE_FC_SUB_MIN" in k


def _params(rows):
    return [pytest.param(k, id=",".join("%s=%s" % kv for kv in k.items()), marks=[pytest.mark.variants] if _VARIANT_KEYS & set(k) else [])
            for k in rows]


ES_FORMS = [k for k in _ES_STEP_KNOBS if _is_sub(k)] + [{"DNE_FC_SUB": "2", "DNE_FC_SUB_MIN": "2", "DNE_FC_SUB_HEAD": "0"}]   # ... + k_out on the chain sums (test_gpu_step_taps.ES_REGIMES "sub_out")
GA_FORMS = [k for k in _GA_STEP_KNOBS if _is_sub(k)]
assert len(ES_FORMS) >= 5 and len(GA_FORMS) >= 2


@functools.lru_cache(maxsize=None)
def _layout():
    return O.layout(O.KIND_ES, NACT)


@functools.lru_cache(maxsize=None)
def _indices():
    """6 pairs: first and last legal slice, every residue mod 4, two overlapping slices; no two closer than the distance of a channel's
    gamma and beta (the edited noise entries of one pair then are no bn2 parameter of channel F_CH in another)"""
    return np.array([0, 1_000_001, 1_000_003, 2_000_002, 64, S.NOISE_LEN - S.P_ES], np.int64)


@functools.lru_cache(maxsize=None)
def _noise():
    """small_noise with, for every pair, channel F_CH's bn2 entries edited: gamma's noise 0, beta's 50 -- sigma * 50 = 1"""
    L, noise = _layout(), S.small_noise().copy()
    for i in _indices():
        noise[i + L.bn2g + F_CH] = 0.0
        noise[i + L.bn2b + F_CH] = 50.0
    for i in _indices():   # (the edits of one pair did not land on another's)
        assert noise[i + L.bn2g + F_CH] == 0.0 and noise[i + L.bn2b + F_CH] == 50.0
    return noise


@functools.lru_cache(maxsize=None)
def _theta(case):
    L, th = _layout(), S.base_theta(KIND_ES).copy()
    th[L.bn2b:L.bn2b + 32] = -BIG
    th[[L.bn2b + c for c in _LIVE[case]]] = BIG
    if case == "split":   # scale 0, shift 0: the members' shifts are +1 and -1, their scales +0 and -0
        th[L.bn2g + F_CH] = 0.0
        th[L.bn2b + F_CH] = 0.0
    return th


def _seeds():
    return S.tap_seeds(2 * len(_indices()))


@functools.lru_cache(maxsize=None)
def _tap(case, m):
    """the oracle's episode of member m under a case's base vector, and the liveness the case was crafted for, from the oracle's own values"""
    sc = np.float32(SIGMA) if m % 2 == 0 else -np.float32(SIGMA)
    th = _theta(case)
    i = int(_indices()[m // 2])
    member = (th + (sc * _noise()[i:i + th.size]).astype(np.float32)).astype(np.float32)
    tap = S.oracle_taps(_layout(), member, S.ref_batch(), int(_seeds()[m]), (T,))[T]
    x = S.activated_y2(tap["y"][1], tap["bn"]).reshape(121, 32)
    live = set(_LIVE[case]) | ({F_CH} if case == "split" and m % 2 == 0 else set())
    for c in range(32):
        assert (x[:, c] > 0).all() if c in live else not x[:, c].any(), (case, m, c)
    return tap


def _same(got, want, *ctx):
    g, w = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = np.flatnonzero(g.view(np.int32) != w.view(np.int32))
    assert bad.size == 0, (ctx, "%d of %d differ, first at %s: %r vs %r" % (bad.size, g.size, bad[:8].tolist(), g[bad[0]], w[bad[0]]))


def _fc_kind(knobs):
    return 4   # profile()["fc_full_kind"]: k_fc_sub


@pytest.mark.parametrize("knobs", _params(ES_FORMS))
def test_dead_rows_by_channel(knobs, monkeypatch):
    """(a) every channel dead: every row of every chain and the over-fetched block read the zero rows, y3 is the fc bias; (b) all live;
    (c) / (d) only channel 0 / 31; (e) the even channels dead; (f) a channel live in member + and dead in member -: the row is fetched"""
    from dne_hip import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    idx, seeds, L = _indices(), _seeds(), _layout()
    n = len(idx)
    e = _lib.Engine(KIND_ES, NACT, max_members=2 * n, ref_count=NREF, record_bc=True, bc_max_steps=T)
    try:
        e.noise_upload(_noise())
        e.set_ref_batch(S.ref_batch())
        for case in CASES:
            e.set_theta(_theta(case))
            ret, sg, ln, bc = e.es_eval(idx, SIGMA, T, seeds, want_bc=True)
            assert (ln == T).all(), (knobs, case, ln.tolist())           # every tap is a lock-step at the full width: the forced kernel
            assert e.profile()["fc_full_kind"] == _fc_kind(knobs), (knobs, case)
            bn = e.get_bn(2 * n)
            ret, sg = ret.reshape(-1), sg.reshape(-1)
            for m in range(2 * n):
                tap = _tap(case, m)
                assert (ret[m], sg[m]) == (tap["ret"], tap["sign"]) and tap["length"] == T, (knobs, case, m)
                assert np.array_equal(bc[m, :T], tap["ram"]), (knobs, case, m, "RAM trajectory", bc[m, :T, 38].tolist(), tap["actions"].tolist())
                _same(bn[m], tap["bn"], knobs, case, m, "bn")
                _, g2, g3 = e.debug_activations(m)
                _same(g2, tap["y"][1], knobs, case, m, "y2")
                _same(g3, tap["y"][2], knobs, case, m, "y3")
                if case == "all_dead" or (case == "split" and m % 2):    # nothing but the bias: member = theta + fl(scale * noise)
                    sc = np.float32(SIGMA) if m % 2 == 0 else -np.float32(SIGMA)
                    i = int(idx[m // 2]) + L.fcb
                    fcb = (_theta(case)[L.fcb:L.fcb + 256] + (sc * _noise()[i:i + 256]).astype(np.float32)).astype(np.float32)
                    _same(g3, fcb, knobs, case, m, "y3 = fc bias")
        assert e.check_redzones() == 0
    finally:
        e.close()


@pytest.mark.parametrize("knobs", _params(ES_FORMS))
def test_dead_rows_short_es_rollout(knobs, monkeypatch):
    """6 pairs x 12 steps on the Xavier start point (about half of every member's rows dead, three in ten in both members)"""
    from dne_hip import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    idx, seeds, L = _indices(), _seeds(), _layout()
    e = _lib.Engine(KIND_ES, NACT, max_members=2 * len(idx), ref_count=NREF)
    try:
        e.noise_upload(_noise())
        e.set_ref_batch(S.ref_batch())
        th = S.base_theta(KIND_ES)
        e.set_theta(th)
        ret, sg, ln = e.es_eval(idx, SIGMA, 12, seeds)
        oret, osg, oln = O.es_eval(L, th, _noise(), idx, SIGMA, 12, S.ref_batch(), seeds)
        assert np.array_equal(ln, oln) and np.array_equal(ret, oret) and np.array_equal(sg, osg), knobs
        assert e.profile()["fc_full_kind"] == _fc_kind(knobs), knobs
    finally:
        e.close()


@pytest.mark.parametrize("knobs", _params(GA_FORMS))
def test_dead_rows_short_ga_rollout(knobs, monkeypatch):
    """k_fc_sub<1, false, false>: 7 written-out children x 12 steps, each skipping on its own relu zeros"""
    from dne_hip import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    noise = S.small_noise()
    e = _lib.Engine(_lib.KIND_GA, NACT, max_members=16, record_bc=True)
    try:
        e.noise_upload(noise)
        L = O.layout(O.KIND_GA, NACT)
        for gen, seeds in zip((S.ga_gen0(), S.ga_gen1()), S.GA_SEEDS):
            ret, sg, ln, bc = e.ga_eval([list(c) for c in gen], S.GA_SIGMA, 12, seeds, want_bc=True)
            for i, chain in enumerate(gen):
                r, s, l, obc = O.rollout(L, O.ga_rebuild(L, noise, list(chain), S.GA_SIGMA), None, seeds[i], 12, want_bc=True)
                assert (ret[i], sg[i], ln[i]) == (r, s, l) and np.array_equal(bc[i], obc), (knobs, i)
    finally:
        e.close()
