"""CPU: the lock-step planner (csrc/plan.h) through dne_debug_plan / dne_debug_knob -- no GPU, no handle.

plan.h decides, from the DNE_* knobs (one table), a few facts about the member set and the active count, everything engine.hip's launchers
do for a window of a burst.  Here: the default regime table, the GPU suite's own mirror of the window cut (test_gpu_step_taps._windows),
that every knob set the GPU suite forces reaches the kernel its comment names, the knob table's clamping and normalisations, and the plan of
dne_act / dne_env_step by member count (dne_debug_plan_act), whose rows tests/test_gpu_frames.py asserts before it launches."""
import os

import pytest

from dne_hip import _lib
import test_gpu_edges as E
import test_gpu_large as TL
import test_gpu_step_taps as T

KIND_ES, KIND_GA, KIND_LARGE = _lib.KIND_ES, _lib.KIND_GA, _lib.KIND_GA_LARGE
NACT = 18
# an ES engine inside dne_es_eval: one base slot, antithetic pairs of one sigma, every buffer there, the whole table covered, four streams
ES_FACTS = dict(uniform_base=1, antithetic_slot0=1, pair_sigma_uniform=1, has_y3s=1, has_theta_perm=1, has_scaled_table=1)
GA_FACTS = dict(members_materialized=1, has_y3s=1)          # Deep-GA children written out (the default)


@pytest.fixture(autouse=True)
def _clean_environment(monkeypatch):
    for k in [k for k in os.environ if k.startswith("DNE_")]:
        monkeypatch.delenv(k)


def _set(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def _fc(row):
    return _lib.FC_NAMES[row.fc]


def _conv(row):
    return _lib.CONV_NAMES[row.conv]


def _plan(kind, total, gsize=None, **facts):
    return _lib.debug_plan(kind, NACT, total, gsize or (2 if kind == KIND_ES else 1), **facts)


def _kind_of(kind, total, **facts):
    return _lib.debug_plan(kind, NACT, total, 2 if kind == KIND_ES else 1, whole_eval=True, **facts)


# ---- 1. the default regime table ------------------------------------------------------------------------------------------------------------
def test_default_es_regime_table():
    """active pairs -> windows, fc kernel and what follows it, with no knob set"""
    def rows(total):
        r = _plan(KIND_ES, total, **ES_FACTS)
        assert sum(w.cnt for w in r) == total and [w.lo for w in r] == [sum(x.cnt for x in r[:i]) for i in range(len(r))]
        return r

    for total in (2500, 1500):      # k_fc_ring on the scaled table behind k_conv12, which leaves relu(bn2(y2)); k_out + k_env_logic / k_env_render
        r = rows(total)
        assert len(r) == 4
        for w in r:
            assert (_fc(w), _conv(w), w.act2, w.ring_scaled, w.head_fused, w.tail, w.spec) == ("k_fc_ring", "k_conv12", 1, 1, 0, 0, 0), total
    for total, nsub in ((1499, 4), (800, 4), (799, 3), (451, 3)):   # k_fc_duo, one unit per wave (below 1500 pairs), raw y2
        r = rows(total)
        assert len(r) == nsub, total
        for w in r:
            assert (_fc(w), w.solo, w.sweep, w.fat, w.act2, w.head_fused) == ("k_fc_duo", 1, 1, 1, 0, 0), total
    for total in (450, 97):         # the sub-slice fc, policy head + emulator in one launch (k_tail_step) behind it
        r = rows(total)
        assert len(r) == 3
        for w in r:
            assert (_fc(w), w.head_fused, w.render_fused, w.tail) == ("k_fc_sub", 1, 0, 0), total
    r = rows(96)                    # 48 + 48 pairs: 96 members are above conv12t_max (64) and below conv_fused_min (129): k_conv1 over 4, k_conv2 over 2
    assert [(w.lo, w.cnt) for w in r] == [(0, 48), (48, 48)]
    for w in r:
        assert (_fc(w), w.tail, w.head_fused, _conv(w), w.s1, w.s2) == ("k_fc_cols", 1, 1, "split", 4, 2)
    r = rows(48)
    assert [(w.lo, w.cnt) for w in r] == [(0, 24), (24, 24)]
    for w in r:
        assert (_fc(w), w.tail, _conv(w)) == ("k_fc_tail", 1, "k_conv12t")
    (w,) = rows(47)
    assert (_fc(w), w.tail, w.spec) == ("k_fc_cols", 1, 0)
    (w,) = rows(4)                  # 8 members > spec_max (4)
    assert (_fc(w), w.tail, w.spec, _conv(w), w.s1, w.s2) == ("k_fc_quad", 1, 0, "k_conv12t", 7, 4)
    (w,) = rows(2)
    assert (_fc(w), w.tail, w.spec) == ("k_fc_quad", 1, 1)
    # the render side of the tail: 8 bands of 512 threads, halved until members x bands fits 512 workgroups; above 192 members 512 threads each
    assert [(rows(t)[0].render_bands, rows(t)[0].render_wg) for t in (2, 32, 47, 96)] == [(8, 512), (8, 512), (4, 512), (4, 512)]
    assert [rows(t)[0].render_wg for t in (451, 97)] == [512, 1024]     # 300 members per window / 64


def test_default_ga_and_large_regime_table():
    for total, fc, nsub in ((321, "k_fc_tail", 4), (320, "k_fc_sub", 4), (97, "k_fc_sub", 4), (96, "k_fc_tail", 2)):
        r = _plan(KIND_GA, total, **GA_FACTS)
        assert len(r) == nsub and all(_fc(w) == fc for w in r), total
    assert all(w.head_fused for w in _plan(KIND_GA, 320, **GA_FACTS))
    # children NOT written out never take the sub-slice fc
    assert all(_fc(w) != "k_fc_sub" for w in _plan(KIND_GA, 320, has_y3s=1))
    # the LargeModel: k_lfc_cols up to 96 members per WINDOW, above it k_lfc<false, 8, 2> (DNE_FC_RB 8 on this kind, DNE_LFC_PAD 2)
    assert _lib.debug_knob(KIND_LARGE, NACT, "DNE_FC_RB") == 8 and _lib.debug_knob(KIND_LARGE, NACT, "DNE_LFC_PAD") == 2
    for total in (96, 97):          # by default two windows of 48 / 49
        r = _plan(KIND_LARGE, total, members_materialized=1)
        assert len(r) == 2 and all((_fc(w), _conv(w), w.s2, w.tail, w.head_fused) == ("k_lfc_cols", "lconv", 4, 0, 0) for w in r)


def test_large_window_of_96_and_97(monkeypatch):
    monkeypatch.setenv("DNE_NSUB", "1")
    assert [_fc(_plan(KIND_LARGE, t, members_materialized=1)[0]) for t in (96, 97)] == ["k_lfc_cols", "k_lfc"]


def test_whole_evaluation_kinds(monkeypatch):
    """dne_profile.fc_full_kind by the width an evaluation starts with: 5 ring, 3 duo, 2 k_fc2, 4 sub, 1 k_fc / the tail kernels"""
    assert [_kind_of(KIND_ES, t, **ES_FACTS) for t in (2500, 1500, 1499, 451, 450, 97, 96, 2)] == [5, 5, 3, 3, 4, 4, 1, 1]
    assert [_kind_of(KIND_GA, t, **GA_FACTS) for t in (1000, 320, 96)] == [1, 4, 1]
    assert _kind_of(KIND_LARGE, 1000, members_materialized=1) == 1
    monkeypatch.setenv("DNE_FC_DUO", "0")
    assert [_kind_of(KIND_ES, t, **ES_FACTS) for t in (2500, 800, 799)] == [2, 2, 1]
    monkeypatch.setenv("DNE_FC2_MIN", "100")        # lowered into the sub-slice fc's range: the evaluation counts as k_fc2's, its bursts run k_fc_sub
    assert _kind_of(KIND_ES, 300, **ES_FACTS) == 2 and all(_fc(w) == "k_fc_sub" for w in _plan(KIND_ES, 300, **ES_FACTS))


# ---- 2. the GPU suite's mirror of the cut ---------------------------------------------------------------------------------------------------
def _mirror_knob_sets():
    sets = [("plain", {}), ("_RING", T._RING), ("_PRODUCT", T._PRODUCT)] + [(n, r[0]) for n, r in T.ES_REGIMES.items()]
    out = []
    for name, knobs in sets:
        out.append(pytest.param(knobs, id=name))
        for k in (1, 2, 3, 4):
            out.append(pytest.param(dict(knobs, DNE_NSUB=str(k)), id="%s-nsub%d" % (name, k)))
    return out


@pytest.mark.parametrize("knobs", _mirror_knob_sets())
def test_step_tap_mirror_matches_the_plan(knobs, monkeypatch):
    """test_gpu_step_taps._windows / _activated_pairs (which rows of an evaluation hold relu(bn2(y2))) against the engine's own plan, for every
    total from 1 to 799.  _windows declares one branch it does not mirror -- the sub-slice fc, whose bursts have DNE_FC_SUB_NSUB windows (it
    refuses DNE_FC_SUB_MIN outright) -- and that is EXACTLY where the two may differ: wherever the plan is not k_fc_sub's, or DNE_NSUB fixes
    the cut, the windows are equal; where it is k_fc_sub's the plan has the regime's three windows and no activated y2.  Under the default
    knobs that is 97 .. 450 pairs, where _windows gives 2 .. 4 windows; the GPU tests consult it only under the ring knobs, which end that range."""
    _set(monkeypatch, knobs)
    mirrored = "DNE_FC_SUB_MIN" not in knobs
    for total in range(1, 800):
        rows = _plan(KIND_ES, total, **ES_FACTS)
        cut = [(w.lo, w.cnt) for w in rows]
        sub = _fc(rows[0]) == "k_fc_sub"
        assert all((_fc(w) == "k_fc_sub") == sub for w in rows)
        assert cut == [(total * s // len(cut), total * (s + 1) // len(cut) - total * s // len(cut)) for s in range(len(cut))], total
        if mirrored and (not sub or "DNE_NSUB" in knobs):
            assert T._windows(total, knobs) == cut, total
        elif sub:
            assert len(cut) == min(int(knobs.get("DNE_NSUB", 3)), total), total
        if mirrored and sub and "DNE_NSUB" not in knobs:
            assert 97 <= total <= 450 and not any(w.act2 for w in rows)
            continue
        act = T._activated_pairs(total, knobs)
        for w in rows:
            assert (act[w.lo:w.lo + w.cnt] == bool(w.act2)).all(), (total, w.lo)


# ---- 3. every knob set of the GPU suite reaches the kernel its comment names -------------------------------------------------------------------
# One entry per row of test_gpu_edges._ES_STEP_KNOBS, in its order: the fc kernel of the WIDEST window at the tests' own populations (5 and
# 11 pairs), fields of that window, and [(total, fields)] checks at other widths.  Written from the rows' comments, not from the plan.
_DUO = dict(act2=0)
_TAIL = dict(tail=1, head_fused=1, spec=0)
_ES_EXPECT = [
    ("k_fc2", {}, []),
    ("k_fc_duo", dict(_DUO, solo=1, head_fused=0), []),
    ("k_fc_duo", dict(_DUO, solo=0), []),
    ("k_fc_duo", dict(_DUO, solo=0, nsub=2), []),
    ("k_fc_duo", dict(_DUO, solo=0), []),
    ("k_fc_duo", dict(_DUO, head_fused=1, render_fused=0), []),
    ("k_fc_duo", dict(_DUO, solo=0, sweep=0), []),
    ("k_fc_duo", dict(_DUO, solo=1, sweep=0), []),
    ("k_fc_duo", dict(_DUO, solo=0, sweep=1), []),
    ("k_fc_sub", dict(head_fused=1), []),
    ("k_fc_sub", dict(nsub=1, sub_spw=2), []),
    ("k_fc_sub", dict(sub_spw=8), []),
    ("k_fc_sub", dict(head_fused=1, render_fused=1), []),
    ("k_fc_duo", dict(_DUO, solo=0, sweep=1, fat=1), []),
    ("k_fc_duo", dict(_DUO, solo=1, sweep=1, fat=1, nsub=2), []),
    ("k_fc_ring", dict(act2=1, ring_scaled=1, conv="k_conv12t"), []),
    ("k_fc_ring", dict(act2=1, ring_scaled=1, conv="k_conv12t"), []),
    ("k_fc_ring", dict(act2=1, conv="k_conv12"), []),
    ("k_fc_ring", dict(act2=1, conv="split", s1=7, s2=4), []),
    ("k_fc_ring", dict(act2=1, nsub=2), []),
    ("k_fc_ring", dict(act2=1, ring_scaled=0), []),
    ("k_fc_tail", _TAIL, []),                                                      # DNE_BURST / DNE_BURST_TAIL: the default kernels
    ("k_fc2", {}, []),
    ("k_fc", {}, []),
    ("k_fc", {}, []),
    ("k_fc_tail", dict(_TAIL, render_fused=0, render_bands=8), [(2, dict(spec=0)), (1, dict(spec=0))]),
    ("k_fc_tail", dict(_TAIL, render_fused=0), [(2, dict(spec=0))]),
    ("k_fc_tail", dict(_TAIL, render_fused=0), [(2, dict(spec=0))]),
    ("k_fc_tail", _TAIL, [(2, dict(spec=1))]),
    ("k_fc_tail", _TAIL, [(2, dict(spec=1))]),
    ("k_fc_tail", _TAIL, [(3, dict(spec=0)), (2, dict(spec=1))]),
    ("k_fc_tail", dict(tail=1, spec=1), [(32, dict(spec=0))]),                      # (never past conv_split_max = 32 members: the 7 / 4 split)
    ("k_fc_tail", dict(tail=0, head_fused=0, spec=0), []),
    ("k_fc_tail", _TAIL, [(1, dict(fc="k_fc_tail"))]),
    ("k_fc_tail", _TAIL, [(1, dict(fc="k_fc_tail"))]),
    ("k_fc_quad", _TAIL, [(1, dict(fc="k_fc_quad"))]),
    ("k_fc_cols", _TAIL, [(1, dict(fc="k_fc_cols"))]),
    ("k_fc_tail", _TAIL, [(4, dict(spec=1, fc="k_fc_quad"))]),
    ("k_fc_tail", dict(_TAIL, render_bands=1, render_fused=1), []),
    ("k_fc_tail", dict(_TAIL, conv="split", s1=7, s2=4), []),
    ("k_fc_tail", dict(_TAIL, conv="split", s1=7, s2=4), []),
    ("k_fc_tail", dict(_TAIL, conv="k_conv12t"), [(47, dict(conv="k_conv12t")), (400, dict(conv="k_conv12t"))]),
    ("k_fc_tail", _TAIL, []),                                                      # DNE_CONV1_FPW / DNE_CONV1_SHARED: the reference pass
    ("k_fc_tail", _TAIL, []),
    ("k_fc_tail", _TAIL, []),
    # DNE_CONV_SPLIT_MAX=0 "4 / 2 workgroups per member instead of 7 / 4": the splits are 4 / 2, but up to 64 members the engine runs k_conv12t
    # (the comment is older than that kernel); k_conv1 / k_conv2 use them from 65 members on
    ("k_fc_tail", dict(_TAIL, conv="k_conv12t", s1=4, s2=2), [(33, dict(conv="split", s1=4, s2=2)), (2, dict(spec=0))]),
    ("k_fc_tail", dict(_TAIL, render_bands=7, render_wg=1024), []),
    (None, dict(nsub=3), [(11, dict(fc="k_fc2")), (7, dict(fc="k_fc2")), (6, dict(fc="k_fc_quad"))]),   # (7 = 2 + 2 + 3: the last window is above DNE_FC_TAIL_MAX)
    ("k_fc_tail", dict(_TAIL, render_bands=2), []),
    ("k_fc_tail", dict(_TAIL, conv="k_conv12"), [(1, dict(conv="k_conv12", spec=1))]),
    # DNE_CONV_FUSED=0 DNE_CONV_SPLIT_MAX=0 "never: separate k_conv1 / k_conv2 launches": k_conv12 never runs, but up to 64 members k_conv12t does
    ("k_fc_tail", dict(_TAIL, conv="k_conv12t"), [(33, dict(conv="split", s1=4, s2=2)), (400, dict(conv="split", s1=1, s2=2))]),   # (three windows of 266 members: conv2 over 2 up to 512)
    ("k_fc_tail", dict(_TAIL, conv="k_conv12t", nsub=1), []),                      # DNE_REF_DEDUP=0: the default plan, only the reference pass differs
]
_GA_EXPECT = [      # test_gpu_edges._GA_STEP_KNOBS at the tests' 7 members
    ("k_fc_tail", dict(_TAIL), []),
    ("k_fc_tail", dict(tail=1, spec=1), []),
    ("k_fc_tail", dict(tail=1), []),
    ("k_fc", {}, []),
    ("k_fc", {}, []),
    ("k_fc", {}, []),
    # "k_fc_cols<1>": written-out children (the default) have no k_fc_cols form -- launch_fc gives them k_fc_quad / k_fc_tail<1, false, false> only,
    # so this row runs k_fc_tail like the next one; children left on the fly do reach k_fc_cols<1> (checked below)
    ("k_fc_tail", dict(_TAIL), []),
    ("k_fc_tail", dict(_TAIL), [(1, dict(fc="k_fc_tail"))]),
    ("k_fc_quad", dict(_TAIL), []),
    ("k_fc_tail", dict(_TAIL, conv="split", s1=7, s2=4), []),
    ("k_fc_sub", dict(head_fused=1, nsub=4), [(2, dict(fc="k_fc_sub"))]),
    ("k_fc_sub", dict(sub_spw=4, nsub=3), []),
    ("k_fc_tail", dict(_TAIL), []),
]


def _check_window(w, nsub, want, ctx):
    for field, value in want.items():
        got = nsub if field == "nsub" else _fc(w) if field == "fc" else _conv(w) if field == "conv" else getattr(w, field)
        assert got == value, (ctx, field, got, value)


def _check_expectation(kind, facts, knobs, populations, expect):
    fc, fields, others = expect
    for total in populations:
        rows = _plan(kind, total, **facts)
        widest = max(rows, key=lambda w: w.cnt)
        if fc is not None:
            assert _fc(widest) == fc, (knobs, total, _fc(widest))
        _check_window(widest, len(rows), fields, (knobs, total))
    for total, want in others:
        rows = _plan(kind, total, **facts)
        _check_window(max(rows, key=lambda w: w.cnt), len(rows), want, (knobs, total))


assert len(_ES_EXPECT) == len(E._ES_STEP_KNOBS) and len(_GA_EXPECT) == len(E._GA_STEP_KNOBS)


@pytest.mark.parametrize("i", range(len(E._ES_STEP_KNOBS)))
def test_es_step_knobs_select_what_their_comments_say(i, monkeypatch):
    knobs = E._ES_STEP_KNOBS[i]
    _set(monkeypatch, knobs)
    _check_expectation(KIND_ES, ES_FACTS, knobs, (5, 11), _ES_EXPECT[i])
    kind = _kind_of(KIND_ES, 11, **ES_FACTS)
    assert kind == T._fc_full_kind(knobs), knobs                      # what test_es_step_knob_taps asserts on the GPU
    for name, value in (("DNE_BURST", 5), ("DNE_BURST_TAIL", 40), ("DNE_FC_RB", 2), ("DNE_HEAD_THREADS", 256), ("DNE_SPEC_CONV1", 0), ("DNE_SPEC_BANDS", 2),
                        ("DNE_CONV1_FPW", None), ("DNE_CONV1_SHARED", 0), ("DNE_REF_DEDUP", 0), ("DNE_TAIL_TABLE", 0), ("DNE_DUO_LAG", 3), ("DNE_BAND_THREADS", 1024)):
        if name in knobs:
            assert _lib.debug_knob(KIND_ES, NACT, name) == (int(knobs[name]) if value is None else value), (knobs, name)


@pytest.mark.parametrize("name", list(T.ES_REGIMES))
def test_es_regimes_select_what_their_comments_say(name, monkeypatch):
    """ES_REGIMES at 11 pairs: the profiled kind the GPU test asserts, and for the tail rows (kind None there: nothing on the GPU checks that the
    knobs reach their kernel) the kernel itself"""
    knobs, fc_kind, y1_written, _ = T.ES_REGIMES[name]
    _set(monkeypatch, knobs)
    rows = _plan(KIND_ES, 11, **ES_FACTS)
    if fc_kind is not None:
        assert _kind_of(KIND_ES, 11, **ES_FACTS) == fc_kind
        assert {_fc(w) for w in rows} == {{5: "k_fc_ring", 4: "k_fc_sub", 3: "k_fc_duo"}[fc_kind]}
    assert all((_conv(w) == "split") == bool(y1_written) for w in rows)      # only the unfused k_conv1 writes y1 inside an evaluation
    want = {"ring_product": dict(conv="k_conv12", act2=1, ring_scaled=1, head_fused=0), "ring_product_nsub2": dict(nsub=2, conv="k_conv12"),
            "ring_product_nsub3": dict(nsub=3), "ring_product_burst4": dict(ring_scaled=1), "ring_conv12t": dict(conv="k_conv12t", act2=1),
            "ring_conv1_conv2": dict(s1=7, s2=4, act2=1), "ring_unscaled": dict(ring_scaled=0, act2=1), "duo": dict(solo=1, conv="k_conv12t"),
            "sub": dict(head_fused=1, conv="k_conv12t"), "sub_out": dict(head_fused=0),
            "tail_default": dict(_TAIL, fc="k_fc_tail", conv="k_conv12t", nsub=1), "tail_default_burst4": dict(_TAIL, fc="k_fc_tail"),
            "tail_spec": dict(spec=1, tail=1), "tail_spec_burst4": dict(spec=1), "tail_fc_quad": dict(_TAIL, fc="k_fc_quad"),
            "tail_fc_tail": dict(_TAIL, fc="k_fc_tail"), "tail_fc_cols": dict(_TAIL, fc="k_fc_cols"), "tail_one_window": dict(nsub=1)}[name]
    for w in rows:
        _check_window(w, len(rows), want, name)
    if name.endswith("burst4"):
        assert _lib.debug_knob(KIND_ES, NACT, "DNE_BURST_TAIL") == 4
    if name == "tail_one_window":                                    # 65 pairs in ONE window: 130 members reach k_conv12 through its default gate
        (w,) = _plan(KIND_ES, 65, **ES_FACTS)
        assert (_conv(w), _fc(w)) == ("k_conv12", "k_fc_cols")
        monkeypatch.delenv("DNE_NSUB")
        assert [(w.cnt, _conv(w), _fc(w)) for w in _plan(KIND_ES, 65, **ES_FACTS)] == [(32, "k_conv12t", "k_fc_tail"), (33, "split", "k_fc_cols")]


@pytest.mark.parametrize("i", range(len(E._GA_STEP_KNOBS)))
def test_ga_step_knobs_select_what_their_comments_say(i, monkeypatch):
    knobs = E._GA_STEP_KNOBS[i]
    _set(monkeypatch, knobs)
    materialize = _lib.debug_knob(KIND_GA, NACT, "DNE_GA_MATERIALIZE")
    assert materialize == int(knobs.get("DNE_GA_MATERIALIZE", "1"))
    facts = dict(members_materialized=materialize, has_y3s=int(_lib.debug_knob(KIND_GA, NACT, "DNE_FC_SUB") != 0))   # (what dne_create allocates)
    _check_expectation(KIND_GA, facts, knobs, (7,), _GA_EXPECT[i])
    if "DNE_FC_RB" in knobs:
        assert _lib.debug_knob(KIND_GA, NACT, "DNE_FC_RB") == 8
    if knobs == {"DNE_SPEC_MAX": "0", "DNE_FC_QUAD_MAX": "0", "DNE_FC_TAILK_MAX": "0"}:
        assert _fc(_plan(KIND_GA, 7, has_y3s=1)[0]) == "k_fc_cols"   # children on the fly


def _large_cases():
    mark = [m for m in TL.test_genomes_evaluated_bit_exact.pytestmark if m.name == "parametrize"][0]
    out = [(6, dict(k, DNE_GA_MATERIALIZE=m)) for m, k in mark.args[1]]
    return out + [tuple(p.values) for p in T._LARGE_CASES]


@pytest.mark.parametrize("n,knobs", _large_cases())
def test_large_model_knobs_select_what_their_comments_say(n, knobs, monkeypatch):
    _set(monkeypatch, knobs)
    materialize = _lib.debug_knob(KIND_LARGE, NACT, "DNE_GA_MATERIALIZE")
    assert materialize == int(knobs.get("DNE_GA_MATERIALIZE", "1"))
    rows = _plan(KIND_LARGE, n, members_materialized=materialize)
    one = knobs.get("DNE_NSUB") == "1"
    assert len(rows) == (1 if one or n < 48 else 2)
    for w in rows:
        streamed = "DNE_LFC_COLS_MAX" in knobs or w.cnt > 96
        assert _fc(w) == ("k_lfc" if streamed else "k_lfc_cols"), (n, knobs)
        assert (_conv(w), w.s2) == ("lconv", 4 if w.cnt <= 128 else 2 if w.cnt <= 256 else 1)     # k_lconv_mfma's tiling ns
        assert (w.tail, w.spec, w.head_fused) == (0, 0, 0)
    # k_lfc<false, 8, PAD> on written-out children: the row batch and the padding the comments name
    assert _lib.debug_knob(KIND_LARGE, NACT, "DNE_FC_RB") == 8
    assert _lib.debug_knob(KIND_LARGE, NACT, "DNE_LFC_PAD") == int(knobs.get("DNE_LFC_PAD", "2"))


# ---- 4. the knob table ------------------------------------------------------------------------------------------------------------------------
def _table():
    """(name, lo, hi) of every row of KNOBS, through the tool that prints DESIGN.md section 11 from plan.h"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "knob_table.py")], capture_output=True, text=True, check=True).stdout
    rows = []
    for line in out.splitlines():
        if line.startswith("| `DNE_"):
            name, default, rng = [c.strip() for c in line.split("|")[1:4]]
            lo, hi = [eval(x, {"__builtins__": {}}) for x in rng.split(" .. ")]
            rows.append((name.strip("`"), eval(default, {"__builtins__": {}}), lo, hi))
    return rows, out


def test_knob_table_clamps_and_design_is_current(monkeypatch):
    rows, out = _table()
    assert len(rows) == 61 and len({r[0] for r in rows}) == 61
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    assert out.strip() in design                                     # section 11 is the tool's output
    snapped = {"DNE_HEAD_THREADS", "DNE_RENDER_THREADS", "DNE_BAND_THREADS", "DNE_FC_SUB_SPW"}
    per_kind = {"DNE_FC_SUB": (2, 1), "DNE_FC_SUB_MAX": (450, 320), "DNE_FC_SUB_NSUB": (3, 4), "DNE_FC_SUB_GRID": (1 << 20, 512), "DNE_GA_MATERIALIZE": (0, 1)}
    for name, default, lo, hi in rows:
        assert _lib.debug_knob(KIND_ES, 17, "no such knob") == -1
        if name not in per_kind:
            assert _lib.debug_knob(KIND_ES, NACT, name) == _lib.debug_knob(KIND_GA, NACT, name) == default, name
        else:
            assert (_lib.debug_knob(KIND_ES, NACT, name), _lib.debug_knob(KIND_GA, NACT, name)) == per_kind[name], name
        if name in snapped or name == "DNE_GA_MATERIALIZE":
            continue
        for kind in (KIND_ES, KIND_GA, KIND_LARGE):
            monkeypatch.setenv(name, str(lo - 7))
            assert _lib.debug_knob(kind, NACT, name) == lo, name
            monkeypatch.setenv(name, str(min(hi + 7, 2 ** 31 - 1)))
            assert _lib.debug_knob(kind, NACT, name) == hi, name
            monkeypatch.setenv(name, str(lo))
            assert _lib.debug_knob(kind, NACT, name) == lo, name
        monkeypatch.delenv(name)


def test_knob_normalisations_and_their_order(monkeypatch):
    knob = lambda kind, name, nact=NACT: _lib.debug_knob(kind, nact, name)
    for value, want in (("300", 256), ("319", 256), ("320", 320), ("9999", 320), ("0", 256)):
        monkeypatch.setenv("DNE_HEAD_THREADS", value)
        assert knob(KIND_ES, "DNE_HEAD_THREADS") == want
    for name in ("DNE_BAND_THREADS", "DNE_RENDER_THREADS"):
        for value, want in (("700", 512), ("511", 256), ("512", 512), ("1023", 512), ("1024", 1024), ("5000", 1024), ("1", 256)):
            monkeypatch.setenv(name, value)
            assert knob(KIND_ES, name) == want, (name, value)
    for value, want in (("3", 0), ("1", 1), ("2", 2), ("4", 4), ("5", 0), ("8", 8), ("9", 8), ("-1", 0)):
        monkeypatch.setenv("DNE_FC_SUB_SPW", value)
        assert knob(KIND_GA, "DNE_FC_SUB_SPW") == want, value
    # per-kind defaults come BEFORE the environment ...
    assert [knob(k, "DNE_FC_RB") for k in (KIND_ES, _lib.KIND_ES_VBN, KIND_GA, KIND_LARGE)] == [4, 4, 4, 8]
    monkeypatch.setenv("DNE_FC_RB", "2")
    assert [knob(k, "DNE_FC_RB") for k in (KIND_ES, KIND_LARGE)] == [2, 2]
    assert [(knob(k, "DNE_FC_SUB"), knob(k, "DNE_FC_SUB_MAX"), knob(k, "DNE_FC_SUB_NSUB")) for k in (KIND_ES, _lib.KIND_ES_VBN, KIND_GA, KIND_LARGE)] == \
        [(2, 450, 3), (2, 450, 3), (1, 320, 4), (1, 320, 4)]
    monkeypatch.setenv("DNE_FC_SUB_NSUB", "2")
    assert knob(KIND_ES, "DNE_FC_SUB_NSUB") == knob(KIND_GA, "DNE_FC_SUB_NSUB") == 2
    # ... and what a kind cannot do AFTER it
    assert [knob(k, "DNE_GA_MATERIALIZE") for k in (KIND_ES, KIND_GA, KIND_LARGE)] == [0, 1, 1]
    monkeypatch.setenv("DNE_GA_MATERIALIZE", "1")
    assert [knob(k, "DNE_GA_MATERIALIZE") for k in (KIND_ES, _lib.KIND_ES_VBN, KIND_GA)] == [0, 0, 1]
    monkeypatch.setenv("DNE_GA_MATERIALIZE", "0")
    assert knob(KIND_GA, "DNE_GA_MATERIALIZE") == 0
    # the speculative tail's candidate arrays hold 30 actions; the engine itself is never wider than 18
    assert [knob(KIND_ES, "DNE_SPEC_MAX", nact) for nact in (2, 18, 30, 31)] == [4, 4, 4, 0]
    monkeypatch.setenv("DNE_SPEC_MAX", "64")
    assert [knob(KIND_ES, "DNE_SPEC_MAX", nact) for nact in (18, 31)] == [64, 0]
    assert _plan(KIND_ES, 2, **ES_FACTS)[0].spec == 1 and _lib.debug_plan(KIND_ES, 31, 2, 2, **ES_FACTS)[0].spec == 0


# ---- 5. the plan of dne_act / dne_env_step (act_window: one window of single members, outside any evaluation) -----------------------------------
def _act(kind, n, nact=NACT, **facts):
    w = _lib.debug_plan_act(kind, nact, n, **facts)
    assert (w.lo, w.cnt, w.tail, w.spec, w.head_fused, w.render_fused, w.act2, w.chain) == (0, n, 0, 0, 0, 0, 0, 0), n   # no fused tail of any kind, raw y2
    return w


def _act_row(kind, n, **facts):
    w = _act(kind, n, **facts)
    return (n, _conv(w), (w.s1, w.s2) if _conv(w) == "split" else None, _fc(w))


def test_act_plan_default_rows():
    """the member counts at which an act changes kernels, READ from the knobs; the rows they give are frames_support.ACT_ROWS, the literals
    tests/test_gpu_frames.py asserts before it launches anything"""
    import frames_support as F
    knob = lambda name: _lib.debug_knob(KIND_ES, NACT, name)
    tailk, c12t, tail, fused = knob("DNE_FC_TAILK_MAX"), knob("DNE_CONV12T_MAX"), knob("DNE_FC_TAIL_MAX"), knob("DNE_CONV_FUSED_MIN")
    assert tailk < c12t < tail < fused - 1 <= knob("DNE_CONV_SPLIT_MID") and knob("DNE_CONV_SPLIT_MAX") < c12t and knob("DNE_FC_QUAD_MAX") < tailk
    counts = (tailk, tailk + 1, c12t, c12t + 1, tail, tail + 1, fused - 1, fused, fused + 2)
    want = ((counts[0], "k_conv12t", None, "k_fc_tail"), (counts[1], "k_conv12t", None, "k_fc_cols"), (counts[2], "k_conv12t", None, "k_fc_cols"),
            (counts[3], "split", (4, 2), "k_fc_cols"), (counts[4], "split", (4, 2), "k_fc_cols"), (counts[5], "split", (4, 2), "k_fc"),
            (counts[6], "split", (4, 2), "k_fc"), (counts[7], "k_conv12", None, "k_fc"), (counts[8], "k_conv12", None, "k_fc"))
    assert want == F.ACT_ROWS                                        # (the defaults are the ones the GPU cases were written for)
    for kind in (KIND_ES, _lib.KIND_ES_VBN, KIND_GA):
        assert tuple(_act_row(kind, n, **F.act_facts()) for n in counts) == want, kind
        assert [_fc(_act(kind, n)) for n in (1, knob("DNE_FC_QUAD_MAX"), knob("DNE_FC_QUAD_MAX") + 1)] == ["k_fc_quad", "k_fc_quad", "k_fc_tail"]
        assert _act_row(kind, 131, nact=3, **F.act_facts()) == (131, "k_conv12", None, "k_fc")
    # the act plan is plan_window under the empty plan: facts an evaluation's burst reads (pairs, the ring's buffers) change nothing ...
    for n in counts:
        a, b = _act(KIND_ES, n), _act(KIND_ES, n, **ES_FACTS)
        assert all(getattr(a, f) == getattr(b, f) for f, _ in _lib.WindowPlan._fields_ if f != "reserved"), n
    # ... and GA children written out (an act right behind dne_ga_eval, before any dne_set_members) have no k_fc_cols form
    assert [_fc(_act(KIND_GA, n, **GA_FACTS)) for n in (tailk, tailk + 1, tail, tail + 1)] == ["k_fc_tail", "k_fc_tail", "k_fc_tail", "k_fc"]
    # the render side of dne_env_step: one workgroup per member, 1024 threads up to 192 members
    assert [(_act(KIND_ES, n).render_bands, _act(KIND_ES, n).render_wg) for n in (32, 192, 193)] == [(1, 1024), (1, 1024), (1, 512)]


def test_act_plan_knob_rows(monkeypatch):
    import frames_support as F
    assert [(k, n) for k, n, *_ in F.ACT_KNOB_ROWS] == [({"DNE_CONV12T_MAX": "0"}, 32), ({"DNE_CONV_FUSED": "0"}, 257)]
    for knobs, n, conv, split, fc in F.ACT_KNOB_ROWS:
        assert _act_row(KIND_ES, n, **F.act_facts())[1] != conv     # (without the knob: k_conv12t / k_conv12)
        with monkeypatch.context() as m:
            _set(m, knobs)
            assert _act_row(KIND_ES, n, **F.act_facts()) == (n, conv, split, fc), knobs
    assert [(r[2], r[3]) for r in F.ACT_KNOB_ROWS] == [("split", (7, 4)), ("split", (1, 2))]


def test_act_plan_large_rows():
    import frames_support as F
    cols = _lib.debug_knob(KIND_LARGE, NACT, "DNE_LFC_COLS_MAX")
    counts = (cols, cols + 1, 129, 257)                             # (k_lconv1 / k_lconv_mfma's 128 and 256 are no knobs)
    rows = []
    for n in counts:
        w = _act(KIND_LARGE, n, **F.act_facts())
        assert _conv(w) == "lconv" and w.s1 == w.s2
        rows.append((n, w.s1, _fc(w)))
    assert tuple(rows) == F.ACT_LARGE_ROWS == ((96, 4, "k_lfc_cols"), (97, 4, "k_lfc"), (129, 2, "k_lfc"), (257, 1, "k_lfc"))
    assert [_act(KIND_LARGE, n).s1 for n in (128, 256)] == [4, 2]
    # single members never take the pair kernel, whatever the member set looks like
    assert _fc(_act(KIND_LARGE, 98, antithetic_slot0=1, uniform_base=1)) == "k_lfc"


def test_act_plan_refuses_what_dne_act_refuses():
    with pytest.raises(_lib.DneError, match="MAZE"):
        _lib.debug_plan_act(_lib.KIND_MAZE, 2, 8)
    with pytest.raises(_lib.DneError, match="at least 1"):
        _lib.debug_plan_act(KIND_ES, NACT, 0)
