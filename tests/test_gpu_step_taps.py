"""GPU: every lock-step kernel regime checked VALUE BY VALUE, not through the argmax of the logits.

The numerics contract (fp32 forward pass bit-exact against the CPU oracle, operation order included) is checked on y1 / y2 / y3 / logits by
tests/test_gpu_parity.py for the kernels dne_act launches (the empty StepPlan).  The kernels that carry the product's time are reached only
from inside an evaluation (plan_step), where the other tests see them through returns, lengths and RAM trajectories -- a filter whose
closest decision is ~400 ulp of the top logit away from flipping.  Here each regime is forced onto a small population (the knobs of
test_every_step_kernel_variant_is_bit_exact, set before Engine(...)), evaluated for T lock-steps, and every compared member's rows are
read back with debug_activations(): inside an evaluation every policy head (k_out, k_tail_step, k_tail_select[_conv1], k_fc, k_fc2)
stores y3[member] (fc output, bias added, before batch norm / relu) and every convolution path y2[member]; finished members are skipped,
so the rows hold the member's LAST lock-step.  They must equal, bit for bit, what tests/step_tap_support.py steps out of the oracle
(pinned to oracle.rollout by tests/test_step_tap_cpu.py).  lengths == T is ASSERTED for every member: every tap then provably comes from a
lock-step at the full list width, i.e. from the forced regime.  T = 1 is a burst's first lock-step (the speculative tail's `fresh`
path), 3 lies inside a burst, 9 with DNE_BURST / DNE_BURST_TAIL = 4 lies behind two compactions.

In the ring regime the y2 row holds relu(bn2(y2)) (k_conv12 with act2, or k_y2_activate); y1 is written inside an evaluation only by the
unfused k_conv1.  The logits are not tapped inside an evaluation (that would add an argument to the hot kernels): the head's arithmetic
behind y3 (bn3 + relu, the output layer's summation order, the bias, the first-maximum argmax and the lane that commits it) is pinned to one
ulp, ties included, by tests/test_gpu_knife_edge.py -- every regime of this file on members whose step-T decision flips between two
noise tables one float32 ulp apart.  The outcome checks (returns / sign-returns / lengths) are repeated here.

Every population here is 18 actions wide.  The helpers take the width (nact) and, on engines that record RAM trajectories, compare every
step's RAM: tests/test_gpu_action_widths.py runs the regimes through them at 3, 4, 9 and 17 actions."""
import numpy as np
import pytest

import step_tap_support as S
from step_tap_support import NACT, NREF, KIND_ES, KIND_ES_VBN
from test_gpu_edges import _ES_STEP_KNOBS, _GA_STEP_KNOBS, _VARIANT_KEYS

pytestmark = pytest.mark.gpu

_RING = {"DNE_FC_DUO_MIN": "2", "DNE_FC_TAIL_MAX": "1"}
_PRODUCT = dict(_RING, DNE_FC_RING="1", DNE_DUO_SOLO_BELOW="0", DNE_RING_MIN="0", DNE_CONV_FUSED_MIN="1")
_ALL_SIGMAS = (0.02, 0.05, 0.0)    # 0.05 on the same engine after 0.02: the scaled copy is rebuilt; 0.0: every member is theta itself

# id -> (knobs, profile()["fc_full_kind"] or None, y1 written, sigmas) -- the kernels each id taps:
ES_REGIMES = {
    # k_conv12<ES>(act2) + k_unit_order + k_fc_ring<true, 8> (k_scale_table's copy) + k_out<2, true>: the 2500-pair product step
    "ring_product": (_PRODUCT, 5, False, _ALL_SIGMAS),
    # ... two / three windows, each with its own unit order and stream
    "ring_product_nsub2": (dict(_PRODUCT, DNE_NSUB="2"), 5, False, _ALL_SIGMAS),
    "ring_product_nsub3": (dict(_PRODUCT, DNE_NSUB="3"), 5, False, _ALL_SIGMAS),
    # ... the active list compacted every 4 lock-steps: T = 9 lies behind two compactions
    "ring_product_burst4": (dict(_PRODUCT, DNE_BURST="4", DNE_BURST_TAIL="4"), 5, False, _ALL_SIGMAS),
    # k_conv12t<ES> + k_y2_activate + k_fc_ring<true> + k_out<2>
    "ring_conv12t": (dict(_RING, DNE_FC_RING="2"), 5, False, _ALL_SIGMAS),
    # k_conv1 (7 workgroups per member) + k_conv2 (4) + k_y2_activate + k_fc_ring<true> + k_out<2>; y1 is written
    "ring_conv1_conv2": (dict(_RING, DNE_FC_RING="2", DNE_CONV_FUSED="0", DNE_CONV12T_MAX="0"), 5, True, _ALL_SIGMAS),
    # k_fc_ring<false, 8>: no scaled copy, the ring multiplies its rows by sigma itself
    "ring_unscaled": (dict(_RING, DNE_FC_RING="2", DNE_RING_PRE="0"), 5, False, _ALL_SIGMAS),
    # k_conv12t + k_unit_order + k_fc_duo (one unit per wave: the default below 1500 pairs) + k_out<2>
    "duo": (_RING, 3, False, (0.02,)),
    # k_conv12t + k_fc_sub<2, true, true> + k_tail_step (folds the chain sums)
    "sub": ({"DNE_FC_SUB": "2", "DNE_FC_SUB_MIN": "2"}, 4, False, _ALL_SIGMAS),
    # ... + k_out<2, true> on the chain sums + k_env_logic
    "sub_out": ({"DNE_FC_SUB": "2", "DNE_FC_SUB_MIN": "2", "DNE_FC_SUB_HEAD": "0"}, 4, False, _ALL_SIGMAS),
    # the default tail at 11 pairs: k_conv12t + k_fc_tail<2, true> + k_tail_step
    "tail_default": ({}, None, False, (0.02,)),
    "tail_default_burst4": ({"DNE_BURST_TAIL": "4"}, None, False, (0.02,)),
    # the speculative tail (default up to 2 pairs, here at every count): k_conv1_spec + k_conv2 (T = 1: fresh), k_conv2_spec on the candidate
    # y1 rows, k_fc_quad_spec<2, true>, k_tail_select_conv1 / k_tail_select (a burst's last lock-step)
    "tail_spec": ({"DNE_SPEC_MAX": "64"}, None, False, (0.02,)),
    "tail_spec_burst4": ({"DNE_SPEC_MAX": "64", "DNE_BURST_TAIL": "4"}, None, False, (0.02,)),
    # no speculation: k_fc_quad<2, true> / k_fc_tail<2, true> / k_fc_cols<2, true> + k_tail_step
    "tail_fc_quad": ({"DNE_SPEC_MAX": "0", "DNE_FC_QUAD_MAX": "64"}, None, False, (0.02,)),
    "tail_fc_tail": ({"DNE_SPEC_MAX": "0", "DNE_FC_QUAD_MAX": "0"}, None, False, (0.02,)),
    "tail_fc_cols": ({"DNE_SPEC_MAX": "0", "DNE_FC_QUAD_MAX": "0", "DNE_FC_TAILK_MAX": "0"}, None, False, (0.02,)),
    # the default kernels with the whole list in one window (at 65 pairs: 130 members reach k_conv12<ES> through its DEFAULT gate)
    "tail_one_window": ({"DNE_NSUB": "1"}, None, False, (0.02,)),
}
# ModelVirtualBN (no conv / fc biases: the opt_off / opt_bias paths of every head and fc kernel): the product ring step, k_fc_duo, k_fc_sub and
# every form of the default tail (speculative; k_fc_quad / k_fc_tail / k_fc_cols + k_tail_step), + k_fc_ring<false> and the burst-of-4 forms
VBN_REGIMES = ("ring_product", "ring_product_burst4", "ring_unscaled", "duo", "sub", "sub_out", "tail_default", "tail_default_burst4",
               "tail_spec", "tail_spec_burst4", "tail_fc_quad", "tail_fc_tail", "tail_fc_cols")


def _ulp_report(got, want):
    g, w = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = np.flatnonzero(g.view(np.int32) != w.view(np.int32))
    if bad.size == 0:
        return "equal"
    key = lambda a: np.where(a.view(np.int32) < 0, np.int64(-2 ** 31) - a.view(np.int32).astype(np.int64), a.view(np.int32).astype(np.int64))
    ulp = np.abs(key(g[bad]) - key(w[bad]))
    return "%d of %d differ, max %d ulp, first at %s: %r vs %r" % (bad.size, g.size, ulp.max(), bad[:8].tolist(), g[bad[0]], w[bad[0]])


def _same(got, want, *ctx):
    assert np.array_equal(got, want), (ctx, _ulp_report(got, want))


def _rows_are_a_permutation(got, want, ctx):
    """got / want: per member a tuple of arrays; every wanted member is exactly one engine row (the GA engines order their members by parent)"""
    free = list(range(len(got)))
    for m, w in enumerate(want):
        hit = [j for j in free if all(np.array_equal(a, b) for a, b in zip(got[j], w))]
        assert hit, (ctx, m, "no engine row holds this member's values")
        free.remove(hit[0])


def _tail_max(knobs):
    return int(knobs.get("DNE_FC_TAIL_MAX", 96))                     # (the engine's default)


def _windows(total, knobs):
    """plan_step's cut of the active list (engine.hip): [(lo, count)] -- only to know which pairs a ring plan hands to k_fc_ring (windows above
    DNE_FC_TAIL_MAX pairs: activated y2) and which to the tail kernels (raw y2).  A SECOND COPY of engine logic, kept to the one branch these
    populations reach (fewer than 800 pairs, no sub-slice fc: DNE_FC2_MIN's nsub_mid and DNE_FC_SUB_NSUB are not mirrored); if plan_step
    changes its cut this must follow -- a stale copy cannot pass quietly: it makes a y2 comparison fail"""
    tail_max = _tail_max(knobs)
    assert total < 800 and "DNE_FC_SUB_MIN" not in knobs
    k = 3 if total > 4 * tail_max else max(2, -(-total // tail_max)) if total >= 48 else 1
    k = max(1, min(int(knobs.get("DNE_NSUB", k)), 4, total))
    return [(total * s // k, total * (s + 1) // k - total * s // k) for s in range(k)]


def _activated_pairs(n_pairs, knobs):
    if knobs.get("DNE_FC_RING", "0") == "0":                         # (the default, DNE_FC_RING=1, needs 1000 pairs: DNE_RING_MIN)
        return np.zeros(n_pairs, bool)
    out = np.zeros(n_pairs, bool)
    for lo, cnt in _windows(n_pairs, knobs):
        out[lo:lo + cnt] = cnt > _tail_max(knobs)
    return out


def _es_engine(kind, knobs, n_pairs, monkeypatch, profile, nact=NACT, record_ram=False, noise=None):
    """record_ram: the engine keeps every member's RAM trajectory (record_bc), max(TAP_STEPS) rows each; noise: another table than small_noise()"""
    from dne_hip import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    e = _lib.Engine(kind, nact, max_members=2 * n_pairs, ref_count=NREF, profile_events=profile,
                    record_bc=record_ram, bc_max_steps=max(S.TAP_STEPS) if record_ram else 0)
    e.noise_upload(S.small_noise() if noise is None else noise)
    e.set_ref_batch(S.ref_batch(nact))
    e.set_theta(S.base_theta(kind, nact))
    return e


def _check_es_eval(e, kind, knobs, idx, seeds, sigma, T, members, y1_written, fc_kind, ctx, nact=NACT, check_ram=False):
    """check_ram (an engine made with record_ram): every compared member's RAM after each of its T steps equals the oracle's -- byte 38 is
    the action of that step's frames, so this pins the argmax of EVERY lock-step, not only what the last one's y3 implies"""
    n = len(idx)
    if check_ram:
        ret, sg, ln, bc = e.es_eval(idx, sigma, T, seeds, want_bc=True)
    else:
        ret, sg, ln = e.es_eval(idx, sigma, T, seeds)
    assert (ln == T).all(), (ctx, ln.tolist())                      # asserted, not filtered: every tap is a lock-step at the full width
    if fc_kind is not None:
        assert e.profile()["fc_full_kind"] == fc_kind, ctx          # the forced regime really ran (5 ring, 4 sub, 3 duo)
    bn = e.get_bn(2 * n)
    act = _activated_pairs(n, knobs)
    ret, sg = ret.reshape(-1), sg.reshape(-1)
    for m in members:
        sc = np.float32(sigma) if m % 2 == 0 else -np.float32(sigma)
        tap = S.es_member_taps(kind, int(idx[m // 2]), float(sc), int(seeds[m]), nact)[T]
        assert (ret[m], sg[m]) == (tap["ret"], tap["sign"]) and tap["length"] == T, (ctx, m)
        if check_ram:
            assert tap["ram"].shape == (T, 128) and np.array_equal(tap["ram"][:, 38], tap["actions"]), (ctx, m)
            assert np.array_equal(bc[m, :T], tap["ram"]), (ctx, m, "RAM trajectory", bc[m, :T, 38].tolist(), tap["actions"].tolist())
        _same(bn[m], tap["bn"], ctx, m, "bn")
        o1, o2, o3 = tap["y"]
        g1, g2, g3 = e.debug_activations(m)
        _same(g2, S.activated_y2(o2, tap["bn"]) if act[m // 2] else o2, ctx, m, "relu(bn2(y2))" if act[m // 2] else "y2")
        _same(g3, o3, ctx, m, "y3")
        if y1_written:
            _same(g1, o1, ctx, m, "y1")
        elif y1_written is None:                                    # a fused convolution kernel ran: nobody wrote this step's y1
            assert not np.array_equal(g1, o1), (ctx, m, "y1 was written: the unfused k_conv1 ran")
    if sigma == 0.0:                                                # both members of a pair are theta itself on the same episode
        for p in range(n):
            a, b = e.debug_activations(2 * p), e.debug_activations(2 * p + 1)
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (ctx, p)


def _run_es_regime(kind, name, monkeypatch, nact=NACT, sigmas=None, check_ram=False):
    """sigmas: None = the regime's own list"""
    knobs, fc_kind, y1_written, own_sigmas = ES_REGIMES[name]
    idx = S.edge_indices(S.num_params(kind, nact))
    n = len(idx)
    assert not _activated_pairs(n, knobs).any() or _activated_pairs(n, knobs).all()   # 11 pairs: no window of this population falls to the tail kernels
    e = _es_engine(kind, knobs, n, monkeypatch, fc_kind is not None, nact, check_ram)
    try:
        for sigma in own_sigmas if sigmas is None else sigmas:
            seeds = np.repeat(S.tap_seeds(n), 2) if sigma == 0.0 else S.tap_seeds(2 * n)
            for T in S.TAP_STEPS:
                _check_es_eval(e, kind, knobs, idx, seeds, sigma, T, range(2 * n), y1_written, fc_kind, (name, nact, sigma, T), nact, check_ram)
        assert e.check_redzones() == 0
    finally:
        e.close()


@pytest.mark.parametrize("name", [r for r in ES_REGIMES if r != "tail_one_window"])   # (11 pairs are one window anyway)
def test_es_regime_taps_on_the_edge_indices(name, monkeypatch):
    """every row of ES_REGIMES (its comment names the kernels) on the 11 edge-index pairs: every residue mod 4, 16- and 256-byte aligned
    slices, the first and the last legal slice, one slice twice, slices one float apart, abutting slices; all 22 members compared"""
    _run_es_regime(KIND_ES, name, monkeypatch)


@pytest.mark.parametrize("name", VBN_REGIMES)
def test_vbn_regime_taps_on_the_edge_indices(name, monkeypatch):
    """DNE_KIND_ES_VBN through k_fc_ring<true> / <false>, k_fc_duo, k_fc_sub and their heads (k_out<2>, k_tail_step, k_out<2, SUB>), and through
    the tail every ModelVirtualBN evaluation ends in (k_conv12t, k_fc_quad / k_fc_tail / k_fc_cols + k_tail_step; speculative: k_conv1_spec,
    k_conv2_spec, k_fc_quad_spec, k_tail_select[_conv1]): the kernels' no-bias paths on the kind's own flat layout, against the oracle on
    the expanded vector"""
    _run_es_regime(KIND_ES_VBN, name, monkeypatch)


_WIDTH_CASES = ([(w, r) for w in S.WIDTHS for r in ("tail_default", "ring_product")] + [(w, r) for w in (2, 5, 9) for r in ("duo", "sub")]
                + [(65, "tail_one_window")])


@pytest.mark.parametrize("width,name", _WIDTH_CASES)
def test_es_width_taps(width, name, monkeypatch):
    """widths: 2 pairs (8 units: one full k_fc_ring workgroup; the default path is the speculative tail: k_conv1_spec, k_conv2_spec,
    k_fc_quad_spec, k_tail_select[_conv1]), 5 (20 units: a partial last workgroup; under the ring / duo knobs the first of three windows is
    one pair wide and falls to the tail kernels: raw y2 there, activated y2 in the others; default: k_conv12t + k_fc_tail + k_tail_step),
    9, 33 (66 members, default: k_conv1 over 4 + k_conv2 over 2 workgroups per member, y1 written, + k_fc_cols) and 65 (130 members;
    default: two windows of 32 / 33 pairs -- k_conv12t + k_fc_tail and k_conv1 / k_conv2 + k_fc_cols; in ONE window, DNE_NSUB=1, the 130
    members reach k_conv12 through its default gate, no DNE_CONV_FUSED_MIN; under the ring knobs three windows).  Up to 11 pairs every
    member is compared, above them step_tap_support.sampled_members (>= 16)."""
    _run_es_width(width, name, monkeypatch)


def _run_es_width(width, name, monkeypatch, nact=NACT, check_ram=False):
    knobs, fc_kind, _, _ = ES_REGIMES[name]
    idx = S.width_indices(width, S.num_params(KIND_ES, nact))
    seeds = S.tap_seeds(2 * width)
    y1_written = name == "tail_default" and width == 33              # 65..128 members: the unfused k_conv1 (4 workgroups per member)
    if name == "tail_one_window" and width == 65:                    # 130 members in one window: above k_conv12t's range (64), so a y1 row
        y1_written = None                                            # nobody wrote means k_conv12 ran, through its default gate
    e = _es_engine(KIND_ES, knobs, width, monkeypatch, fc_kind is not None, nact, check_ram)
    try:
        for T in S.TAP_STEPS:
            _check_es_eval(e, KIND_ES, knobs, idx, seeds, 0.02, T, S.sampled_members(idx), y1_written, fc_kind, (name, nact, width, T), nact, check_ram)
    finally:
        e.close()


# mixed scales through set_members + eval_members: groups of one, the non-uniform-sigma path (no pairs: no ring / duo / sub)
_MIXED_OFF = np.array([1_000_000, 1_000_000, 1_000_000, 0, S.NOISE_LEN - S.P_ES], np.int64)   # three members share one offset
_MIXED_SCALE = np.array([0.02, -0.02, 0.0, 0.5, -0.1], np.float32)


@pytest.mark.parametrize("knobs", [{}, {"DNE_SPEC_MAX": "64"}, {"DNE_FC_TAIL_MAX": "1"}], ids=["tail_default", "tail_spec", "k_fc"])
def test_mixed_scale_members_taps(knobs, monkeypatch):
    """five single members of base slot 0 (scales 0.02, -0.02, 0, 0.5, -0.1): k_conv12t + k_fc_tail<1, true> + k_tail_step (default),
    the speculative tail's k_fc_quad_spec<1, true>, and the streaming k_fc<1> (DNE_FC_TAIL_MAX=1)"""
    from dne_hip import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    e = _lib.Engine(_lib.KIND_ES, NACT, max_members=8, ref_count=NREF)
    try:
        e.noise_upload(S.small_noise()); e.set_ref_batch(S.ref_batch()); e.set_theta(S.base_theta(KIND_ES))
        n = len(_MIXED_OFF)
        seeds = S.tap_seeds(n)
        for T in S.TAP_STEPS:
            e.set_members(np.zeros(n, np.int32), _MIXED_OFF, _MIXED_SCALE)
            ret, sg, ln = e.eval_members(n, T, seeds)
            assert (ln == T).all(), (knobs, T, ln.tolist())
            bn = e.get_bn(n)
            for m in range(n):
                tap = S.es_member_taps(KIND_ES, int(_MIXED_OFF[m]), float(_MIXED_SCALE[m]), int(seeds[m]))[T]
                assert (ret[m], sg[m]) == (tap["ret"], tap["sign"]) and tap["length"] == T, (knobs, T, m)
                _same(bn[m], tap["bn"], knobs, T, m, "bn")
                _, g2, g3 = e.debug_activations(m)
                _same(g2, tap["y"][1], knobs, T, m, "y2")
                _same(g3, tap["y"][2], knobs, T, m, "y3")
    finally:
        e.close()


def _es_variant_params():
    """every entry of test_gpu_edges._ES_STEP_KNOBS that is not a row of ES_REGIMES: behind `variants` where it forces a kernel no default
    path launches (the rule of test_gpu_edges._knob_params), else in the default suite"""
    have = [r[0] for r in ES_REGIMES.values()]
    out = []
    for k in _ES_STEP_KNOBS:
        if k in have:
            continue
        ident = ",".join("%s=%s" % kv for kv in k.items())
        out.append(pytest.param(k, id=ident, marks=[pytest.mark.variants] if _VARIANT_KEYS & set(k) else []))
    return out


# the entries of _ES_STEP_KNOBS under which 22 members run the unfused k_conv1 (no k_conv12t, no k_conv12, no speculative tail): y1 is written
_UNFUSED_CONV1 = [{"DNE_SPEC_MAX": "0", "DNE_CONV12T_MAX": "0"}, {"DNE_SPEC_MAX": "0", "DNE_CONV12T_MAX": "0", "DNE_TAIL_TABLE": "0"}]
assert all(k in _ES_STEP_KNOBS for k in _UNFUSED_CONV1)


def _fc_full_kind(knobs):
    """profile()["fc_full_kind"] of an 11-pair evaluation under an _ES_STEP_KNOBS entry (engine.hip: ring 5, else duo 3, else k_fc2 2, else sub 4,
    else 1), from the knob that forces the fc; a wrong expectation here can only make the test fail"""
    if knobs.get("DNE_FC_RING", "0") != "0":
        return 5
    if "DNE_FC_DUO_MIN" in knobs:
        return 3
    if "DNE_FC2_MIN" in knobs:
        return 2
    return 4 if "DNE_FC_SUB_MIN" in knobs else 1


@pytest.mark.parametrize("knobs", _es_variant_params())
def test_es_step_knob_taps(knobs, monkeypatch):
    """the rest of _ES_STEP_KNOBS (each entry's comment in tests/test_gpu_edges.py names its kernels: k_fc2, k_fc<2> with DNE_FC_RB, the
    DNE_DUO_FAT forms, two units per wave, DNE_SUB_RENDER_FUSED, the convolution splits, ...) with the same tap on the edge-index pairs;
    profile()["fc_full_kind"] is the evidence that the forced fc ran (2 = k_fc2, 1 = k_fc / the tail kernels)"""
    idx = S.edge_indices(S.P_ES)
    n = len(idx)
    seeds = S.tap_seeds(2 * n)
    e = _es_engine(KIND_ES, knobs, n, monkeypatch, False)
    try:
        for T in S.TAP_STEPS:   # (fc_full_kind is set by every evaluation, with or without profiling events)
            _check_es_eval(e, KIND_ES, knobs, idx, seeds, 0.02, T, range(2 * n), knobs in _UNFUSED_CONV1, _fc_full_kind(knobs), (knobs, T))
    finally:
        e.close()


# ---- GAAtariPolicy ---------------------------------------------------------------------------------------------------------------------
def _ga_params():
    out = [pytest.param({}, id="default")]    # children written out: k_conv12t<false> + k_fc_tail<1, false, false> + k_tail_step<false>
    for k in _GA_STEP_KNOBS:
        out.append(pytest.param(k, id=",".join("%s=%s" % kv for kv in k.items()), marks=[pytest.mark.variants] if _VARIANT_KEYS & set(k) else []))
    return out


@pytest.mark.parametrize("knobs", _ga_params())
def test_ga_regime_taps(knobs, monkeypatch):
    """KIND_GA (no batch norm): 7 fresh genomes, then 7 children of two of them, roots and mutation seeds from the edge set (slice 0, the
    last legal slice, a multiple of 4, an odd index, one seed for both parents); y2 / y3 after ga_eval at T = 1 and 6 through the default
    path and every entry of test_gpu_edges._GA_STEP_KNOBS, member by member with DNE_GA_SORT=0 (the engine then keeps the caller's member order;
    by default it groups the children by parent slot, a schedule: the default path is run that way too and its rows must be the oracle's
    up to that order) (its comments name the kernels: the noise-free k_fc_quad / k_fc_tail / k_fc_cols
    <1, false, false> on written-out children, parent + noise rows on the fly, k_fc_sub<1, false, false>, the streaming k_fc<1>)"""
    _run_ga_regime(knobs, monkeypatch)


def _run_ga_regime(knobs, monkeypatch, nact=NACT):
    from dne_hip import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    for sort in ("0", "1") if not knobs else ("0",):
        monkeypatch.setenv("DNE_GA_SORT", sort)
        e = _lib.Engine(_lib.KIND_GA, nact, max_members=16, record_bc=True)
        try:
            e.noise_upload(S.small_noise())
            for gen, seeds in zip((S.ga_gen0(nact), S.ga_gen1(nact)), S.GA_SEEDS):
                for T in S.GA_TAP_STEPS:
                    ret, sg, ln, bc = e.ga_eval([list(c) for c in gen], S.GA_SIGMA, T, seeds, want_bc=True)
                    assert (ln == T).all(), (knobs, T, ln.tolist())
                    taps = [S.ga_member_taps(tuple(chain), S.GA_SIGMA, int(seeds[m]), S.GA_TAP_STEPS, nact)[T] for m, chain in enumerate(gen)]
                    for m, tap in enumerate(taps):
                        assert (ret[m], sg[m]) == (tap["ret"], tap["sign"]) and np.array_equal(bc[m], tap["ram"][-1]), (knobs, T, m)
                    rows = [e.debug_activations(m)[1:] for m in range(len(gen))]
                    if sort == "1":
                        _rows_are_a_permutation(rows, [t["y"][1:3] for t in taps], (knobs, T))
                        continue
                    for m, tap in enumerate(taps):
                        _same(rows[m][0], tap["y"][1], knobs, T, gen[m], "y2")
                        _same(rows[m][1], tap["y"][2], knobs, T, gen[m], "y3")
            assert e.check_redzones() == 0
        finally:
            e.close()


# ---- LargeModel ------------------------------------------------------------------------------------------------------------------------
LARGE_TAP_STEPS = S.LARGE_TAP_STEPS


_LARGE_CASES = [
    # 6 members: k_lconv1 + k_lconv_mfma (ns = 4) + k_lfc_cols<false> + k_lout, children written out
    pytest.param(6, {}, id="6-default"),
    pytest.param(6, {"DNE_GA_MATERIALIZE": "0"}, id="6-on_the_fly"),                          # k_lconv_mfma<.., NOISE> + k_lfc_cols<true>
    pytest.param(6, {"DNE_LFC_COLS_MAX": "0"}, id="6-k_lfc"),                                 # k_lfc<false, 8, 2> (padded: one workgroup per CU)
    pytest.param(6, {"DNE_LFC_COLS_MAX": "0", "DNE_LFC_PAD": "1"}, id="6-k_lfc_pad1"),        # k_lfc<false, 8, 1>
    pytest.param(6, {"DNE_LFC_COLS_MAX": "0", "DNE_GA_MATERIALIZE": "0"}, id="6-k_lfc_on_the_fly"),   # k_lfc<true, 4>
    # 130 members, default: two windows of 65 (ns = 4, k_lfc_cols); one window (DNE_NSUB=1): ns = 2 and k_lfc
    pytest.param(130, {}, id="130-default"),
    pytest.param(130, {"DNE_NSUB": "1"}, id="130-one_window_ns2"),
    # 260 members in one window: ns = 1 (one workgroup per member and convolution), k_lfc
    pytest.param(260, {"DNE_NSUB": "1"}, id="260-one_window_ns1"),
]


@pytest.mark.parametrize("n,knobs", _LARGE_CASES)
def test_large_model_taps(n, knobs, oracle, monkeypatch):
    """KIND_GA_LARGE: raw conv1 / conv2 / conv3 outputs and the fc's 512 sums (y1..y4 of debug_activations_large) after ga_eval_powers against
    forward_large_debug on the oracle's episode, for the first, the last and six sampled members (all six at n = 6).  Inside an evaluation the
    active list is cut into windows (plan_step): the tilings ns = 2 / 1 of k_lconv_mfma need more than 128 / 256 members in ONE window,
    which below ~400 members only DNE_NSUB=1 gives."""
    _run_large(n, knobs, monkeypatch)


def _run_large(n, knobs, monkeypatch, nact=NACT):
    """(the genomes, their 9M-entry noise table and the oracle's side: step_tap_support.large_genomes / big_noise / large_member_taps)"""
    from dne_hip import _lib, ga_gpu
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    big_noise = S.big_noise()
    sb = ga_gpu.model_scale_by(nact, _lib.KIND_GA_LARGE)
    genomes = S.large_genomes(n, nact)
    seeds = S.tap_seeds(n)
    pick = sorted({0, n - 1} | set(np.random.RandomState(n).permutation(n)[:6].tolist()))
    taps = {m: S.large_member_taps(n, m, nact) for m in pick}
    # DNE_GA_SORT=0: rows in the caller's member order; the default order (children grouped by parent, a schedule) once, at n = 6 where every
    # member has its oracle rows: the engine's rows must be the oracle's up to that order
    for sort in ("0", "1") if n == 6 and not knobs else ("0",):
        monkeypatch.setenv("DNE_GA_SORT", sort)
        e = _lib.Engine(_lib.KIND_GA_LARGE, nact, max_members=n)
        try:
            e.noise_upload(big_noise)
            e.ga_set_init_scale(sb)
            for T in LARGE_TAP_STEPS:
                ret, sg, ln = e.ga_eval_powers(genomes, T, seeds)
                assert (ln == T).all(), (n, knobs, T)
                for m in pick:
                    assert (ret[m], sg[m]) == (taps[m][T]["ret"], taps[m][T]["sign"]) and taps[m][T]["length"] == T, (n, knobs, T, m)
                if sort == "1":
                    assert pick == list(range(n))
                    _rows_are_a_permutation([e.debug_activations_large(m) for m in range(n)], [taps[m][T]["y"] for m in pick], (n, T))
                    continue
                for m in pick:
                    for name, got, want in zip(("y1", "y2", "y3", "y4"), e.debug_activations_large(m), taps[m][T]["y"]):
                        _same(got, want, n, knobs, T, m, name)
            assert e.check_redzones() == 0
        finally:
            e.close()
