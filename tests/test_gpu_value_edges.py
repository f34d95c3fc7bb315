"""GPU: every forward route against the oracle at the ends of float32's range.

DESIGN.md section 3 claims every forward kernel bit for bit the oracle's fp32 chain, and the rest of the suite pins that along every
structural axis on weights between about 1e-9 and 1e2.  Here the same regimes run on the populations of tests/value_edge_support.py: one
tensor group of the base vector times a power of two, so that the layer behind it straddles FLT_MIN (U1..U4, with a subnormal sigma: the
matrix cores' and the packed-math kernels' subnormal operands and results, k_scale_table's pre-scaled copy) or crosses FLT_MAX half-way
down a chain (O1..O4, BIG: where the chain crosses depends on the summation order; behind it +-inf and NaN meet every relu / bn-relu site,
the dead-row shortcut of k_fc_sub and the first-maximum argmax).  tests/test_value_edges_cpu.py shows from the oracle alone that each class
does that, and that the oracle itself is the written fmaf chain there.

Comparison: value_edge_support.same_bits -- NaN where the oracle has NaN, equal bit patterns everywhere else (the sign of zero and of
infinity count).  Inside an evaluation: bn and the batch moments behind it, y2 (activated where the ring leaves it so), y3, y1 where the
regime writes it, returns, sign-returns, lengths == T, and the RAM trajectory (byte 38 is the action: the argmax over NaN / infinite
logits is held at every step, although logits are not tapped there).  Through dne_act: bn, moments, y1, y2, y3, logits and actions at the
member counts where its plan changes.

Non-finite floats are ordinary data to every kernel here: no value is used as an index, and the argmax lands in 0..nact-1."""
import numpy as np
import pytest

import frames_support as F
import step_tap_support as S
import value_edge_support as V
from step_tap_support import NACT, KIND_ES, KIND_ES_VBN, KIND_GA, KIND_GA_LARGE
from test_gpu_edges import _VARIANT_KEYS
from test_gpu_frames import _route
from test_gpu_step_taps import ES_REGIMES, _activated_pairs, _es_engine

pytestmark = pytest.mark.gpu

_ES_ROWS = [r for r in ES_REGIMES if r != "tail_one_window"]          # (5 pairs are one window anyway)
_VBN_ROWS = ("ring_product", "ring_unscaled", "duo", "sub", "tail_default", "tail_spec")


def _regime_params(kind, rows):
    return [pytest.param(r, c, id="%s-%s" % (r, c), marks=[pytest.mark.variants] if _VARIANT_KEYS & set(ES_REGIMES[r][0]) else [])
            for r in rows for c in V.CLASSES[kind]]


def _check_edge_eval(e, kind, cls, knobs, T, y1_written, fc_kind, ctx):
    """test_gpu_step_taps._check_es_eval on a class's five pairs, with same_bits and every step's RAM"""
    idx = V.pair_indices(kind)
    n = len(idx)
    ret, sg, ln, bc = e.es_eval(idx, V.sigma_of(kind, cls), T, V.SEEDS, want_bc=True)
    assert (ln == T).all(), (ctx, ln.tolist())                      # every tap is a lock-step at the full width
    if fc_kind is not None:
        assert e.profile()["fc_full_kind"] == fc_kind, ctx          # the forced regime really ran
    bn, mom = e.get_bn(2 * n), e.get_bn_moments(2 * n)
    act = _activated_pairs(n, knobs)
    ret, sg = ret.reshape(-1), sg.reshape(-1)
    for m in range(2 * n):
        tap = V.taps(kind, cls, m)[T]
        assert (ret[m], sg[m]) == (tap["ret"], tap["sign"]) and tap["length"] == T, (ctx, m)
        assert tap["ram"].shape == (T, 128) and np.array_equal(tap["ram"][:, 38], tap["actions"]), (ctx, m)
        assert np.array_equal(bc[m, :T], tap["ram"]), (ctx, m, "RAM trajectory", bc[m, :T, 38].tolist(), tap["actions"].tolist())
        V.same_bits(bn[m], tap["bn"], ctx, m, "bn")
        V.same_bits(mom[m], V.moments(kind, cls, m), ctx, m, "bn moments")
        o1, o2, o3 = tap["y"]
        g1, g2, g3 = e.debug_activations(m)
        V.same_bits(g2, S.activated_y2(o2, tap["bn"]) if act[m // 2] else o2, ctx, m, "relu(bn2(y2))" if act[m // 2] else "y2")
        V.same_bits(g3, o3, ctx, m, "y3")
        if y1_written and act[m // 2]:                              # (the one-pair first window of the ring knobs falls to the tail kernels)
            V.same_bits(g1, o1, ctx, m, "y1")


def _run_edge_regime(kind, name, cls, monkeypatch):
    knobs, fc_kind, y1_written, _ = ES_REGIMES[name]
    e = _es_engine(kind, knobs, V.N_PAIRS, monkeypatch, fc_kind is not None, NACT, True)
    try:
        e.set_theta(V.base(kind, cls))
        for T in V.TAPS:
            _check_edge_eval(e, kind, cls, knobs, T, y1_written, fc_kind, (name, cls, T))
        assert e.check_redzones() == 0
    finally:
        e.close()


@pytest.mark.parametrize("name,cls", _regime_params(KIND_ES, _ES_ROWS))
def test_es_regimes_at_the_range_ends(name, cls, monkeypatch):
    """every row of test_gpu_step_taps.ES_REGIMES (its comments name the kernels) x every class"""
    _run_edge_regime(KIND_ES, name, cls, monkeypatch)


@pytest.mark.parametrize("name,cls", _regime_params(KIND_ES_VBN, _VBN_ROWS))
def test_vbn_regimes_at_the_range_ends(name, cls, monkeypatch):
    """ModelVirtualBN (the no-bias paths) through k_fc_ring<true> / <false>, k_fc_duo, k_fc_sub, the default and the speculative tail; the
    class scales the kind's own flat layout, the oracle runs the expanded vector"""
    _run_edge_regime(KIND_ES_VBN, name, cls, monkeypatch)


# ---- GAAtariPolicy -------------------------------------------------------------------------------------------------------------------------
_GA_KNOBS = [pytest.param({}, id="default"),             # children written out: k_materialize_children, then the noise-free kernels
             pytest.param({"DNE_GA_MATERIALIZE": "0"}, id="DNE_GA_MATERIALIZE=0", marks=[pytest.mark.variants])]    # parent + noise rows on the fly


@pytest.mark.parametrize("cls", list(V.CLASSES[KIND_GA]))
@pytest.mark.parametrize("knobs", _GA_KNOBS)
def test_ga_at_the_range_ends(knobs, cls, monkeypatch):
    """seven children of one parent.  The engine forms the parent itself, noise * scale_by with the normc factors (the class's groups times 2^e)
    as scale_by -- first read back against the oracle's vector, bit for bit -- and the children from it with powers of +-0.005 (times 2^e in
    an under class); y2 / y3, returns and the final RAM after 1 and 3 steps, member by member (DNE_GA_SORT=0)"""
    from dne_hip import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DNE_GA_SORT", "0")
    genomes, seeds = V.ga_genomes(cls), V.SEEDS[:V.GA_EVAL_MEMBERS]
    e = _lib.Engine(_lib.KIND_GA, NACT, max_members=16, record_bc=True)
    try:
        e.noise_upload(S.small_noise())
        e.ga_set_init_scale(V.ga_scale_by(cls))
        V.same_bits(e.ga_rebuild_powers(1, V.GA_PARENT), V.base(KIND_GA, cls), knobs, cls, "parent")
        for T in V.TAPS:
            ret, sg, ln, bc = e.ga_eval_powers(genomes, T, seeds, want_bc=True)
            assert (ln == T).all(), (knobs, cls, T, ln.tolist())
            for m in range(len(genomes)):
                tap = V.taps(KIND_GA, cls, m)[T]
                assert (ret[m], sg[m]) == (tap["ret"], tap["sign"]) and tap["length"] == T, (knobs, cls, T, m)
                assert np.array_equal(bc[m], tap["ram"][-1]), (knobs, cls, T, m, "final RAM", int(bc[m, 38]), tap["actions"].tolist())
                _, g2, g3 = e.debug_activations(m)
                V.same_bits(g2, tap["y"][1], knobs, cls, T, m, "y2")
                V.same_bits(g3, tap["y"][2], knobs, cls, T, m, "y3")
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- LargeModel ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", list(V.CLASSES[KIND_GA_LARGE]))
@pytest.mark.parametrize("knobs", [pytest.param({}, id="6-default"), pytest.param({"DNE_GA_MATERIALIZE": "0"}, id="6-on_the_fly")])
def test_large_model_at_the_range_ends(knobs, cls, monkeypatch):
    """the two six-member rows of test_gpu_step_taps._LARGE_CASES (k_lconv1 + k_lconv_mfma + k_lfc_cols + k_lout, children written out / on
    the fly) with scale_by's conv1 or fc group times 2^e: y1..y4 after 1 and 3 steps"""
    from dne_hip import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("DNE_GA_SORT", "0")
    genomes, seeds = V.large_genomes(cls), S.tap_seeds(V.N_LARGE)
    e = _lib.Engine(_lib.KIND_GA_LARGE, NACT, max_members=V.N_LARGE)
    try:
        e.noise_upload(S.big_noise())
        e.ga_set_init_scale(V.large_scale_by(cls))
        for T in V.TAPS:
            ret, sg, ln = e.ga_eval_powers(genomes, T, seeds)
            assert (ln == T).all(), (knobs, cls, T, ln.tolist())
            for m in range(V.N_LARGE):
                tap = V.large_taps(cls, m)[T]
                assert (ret[m], sg[m]) == (tap["ret"], tap["sign"]) and tap["length"] == T, (knobs, cls, T, m)
                for name, got, want in zip(("y1", "y2", "y3", "y4"), e.debug_activations_large(m), tap["y"]):
                    V.same_bits(got, want, knobs, cls, T, m, name)
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- dne_act: the only place logits can be read -----------------------------------------------------------------------------------------------
_ACT_ROWS = [r for r in F.ACT_ROWS if r[0] in (32, 33, 65, 97, 129)]      # k_conv12t / split / k_conv12 x k_fc_tail / k_fc_cols / k_fc, all behind k_out
_ACT_CLASSES = ("U4", "O4", "U3", "O1")
_EDGE_SLOT = 1 + len(F.GA_PARENTS)                                     # GA: the class's parent, behind frames_support's three
assert len(_ACT_ROWS) == 5


@pytest.mark.parametrize("n,conv,split,fc", _ACT_ROWS, ids=[str(r[0]) for r in _ACT_ROWS])
@pytest.mark.parametrize("cls", _ACT_CLASSES)
@pytest.mark.parametrize("kind", [KIND_ES, KIND_GA], ids=["es", "ga"])
def test_act_routes_at_the_range_ends(kind, cls, n, conv, split, fc, oracle, monkeypatch):
    """members 0..9 are the class's population on frames_support's crafted frames and are the ones compared; the rest are filler with
    frames_support's offsets, scales and frames (ES: around the class's base, the engine's one slot-0 vector; GA: around frames_support's own
    parents).  The route is asserted before anything is launched."""
    from dne_hip import _lib
    assert _route(kind, NACT, n) == (conv, split, fc), (F.KIND_NAMES[kind], n)
    e = _lib.Engine(kind, NACT, max_members=n, ref_count=F.NREF)
    try:
        e.noise_upload(S.small_noise())
        slot, off, scale = F.members(kind, NACT, n)
        if kind == KIND_ES:
            e.set_theta(V.base(kind, cls))
            e.set_ref_batch(F.ref_batch())
        else:
            for s, chain in enumerate(F.GA_PARENTS, 1):
                e.ga_rebuild(s, chain, F.GA_SIGMA, copy_out=False)
            e.set_theta(V.base(kind, cls), _EDGE_SLOT)
            slot[:2 * V.N_PAIRS] = _EDGE_SLOT
        for m in range(2 * V.N_PAIRS):
            off[m], scale[m] = V.member(kind, cls, m)
        e.set_members(slot, off, scale)
        e.env_set_observation(F.member_frames(n))
        if kind == KIND_ES:
            e.ref_pass(n)
            bn, mom = e.get_bn(n), e.get_bn_moments(n)
        actions, logits = e.act(n)
        assert logits.shape == (n, NACT) and ((0 <= actions) & (actions < NACT)).all()
        for m in range(2 * V.N_PAIRS):
            want = V.act_expected(kind, cls, m)
            ctx = (F.KIND_NAMES[kind], cls, n, m, F.frame_of(m))
            if kind == KIND_ES:
                V.same_bits(bn[m], want["bn"], ctx, "bn")
                V.same_bits(mom[m], want["mom"], ctx, "bn moments")
            for name, got, w in zip(("y1", "y2", "y3"), e.debug_activations(m), want["y"]):
                V.same_bits(got, w, ctx, name)
            V.same_bits(logits[m], want["logits"], ctx, "logits")
            assert int(actions[m]) == int(want["action"]) == S.argmax_first(want["logits"]), (ctx, int(actions[m]), int(want["action"]))
        assert e.check_redzones() == 0
    finally:
        e.close()
