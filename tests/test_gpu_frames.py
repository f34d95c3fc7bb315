"""GPU: every dne_act route on frames the fixture never draws.

The forward kernels are held to the oracle bit for bit mostly from inside evaluations, whose frames the SynthAtari renderer draws: 208 of
the 256 byte values, channels that mostly agree.  Arbitrary frames come in through env_set_observation + act, and the other tests that do
that stay at 3 .. 24 members, where an act runs k_conv12t and k_fc_quad / k_fc_tail (LargeModel: four workgroups per member, k_lfc_cols).
Here the crafted frames of tests/frames_support.py go through dne_act at every member count at which its plan changes, so they meet

  k_conv12 (its 256-entry byte table, the channel pick, conv1's zero border), k_conv1 + k_conv2 over 1 / 2, 4 / 2 and 7 / 4 workgroups
  per member, k_fc_cols, the streaming k_fc with k_out behind it (also at 3 actions); on the LargeModel k_lconv1 / k_lconv_mfma over 4, 2
  and 1 workgroups per member with their SAME-padding taps, k_lfc_cols and k_lfc.

Each case first asserts the route (dne_debug_plan_act with the engine's facts against frames_support's literal rows: a default that moves
fails the case instead of quietly covering less), then checks EVERY member with np.array_equal: bn and its moments, y1..y3 (y1..y4), the
logits, action == first maximum of the logits == the oracle's action, the frames read back, the red zones.  The oracle side of member i is
the same at every count and worked out once per session.  tests/test_frames_cpu.py runs the same drive / check on the oracle engine."""
import pytest

import frames_support as F
from frames_support import KIND_ES, KIND_ES_VBN, KIND_GA, KIND_GA_LARGE, NACT

pytestmark = pytest.mark.gpu


def _route(kind, nact, n):
    from dne_hip import _lib
    w = _lib.debug_plan_act(kind, nact, n, **F.act_facts())
    conv = _lib.CONV_NAMES[w.conv]
    return conv, (w.s1, w.s2) if conv in ("split", "lconv") else None, _lib.FC_NAMES[w.fc]


def _case(kind, nact, n, route, knobs, monkeypatch):
    """one engine of exactly n members under `knobs`; the route asserted, the case driven, every member checked"""
    from dne_hip import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    assert _route(kind, nact, n) == route, (F.KIND_NAMES[kind], nact, n, knobs)
    e = _lib.Engine(kind, nact, max_members=n, ref_count=F.NREF)
    try:
        e.noise_upload(F.noise_of(kind))
        F.check(F.drive(e, kind, nact, n))
    finally:
        e.close()


@pytest.mark.parametrize("n,conv,split,fc", F.ACT_ROWS, ids=[str(r[0]) for r in F.ACT_ROWS])
@pytest.mark.parametrize("kind", [KIND_ES, KIND_ES_VBN, KIND_GA], ids=["es", "vbn", "ga"])
def test_act_routes_on_crafted_frames(kind, n, conv, split, fc, oracle, monkeypatch):
    _case(kind, NACT, n, (conv, split, fc), {}, monkeypatch)


@pytest.mark.parametrize("knobs,n,conv,split,fc", F.ACT_KNOB_ROWS, ids=["CONV12T_MAX=0-32", "CONV_FUSED=0-257"])
def test_act_knob_routes_on_crafted_frames(knobs, n, conv, split, fc, oracle, monkeypatch):
    """k_conv1 over 7 workgroups per member (conv1_body as the speculative tail runs it) with k_conv2 over 4, and over 1 with k_conv2 over 2"""
    _case(KIND_ES, NACT, n, (conv, split, fc), knobs, monkeypatch)


def test_act_at_three_actions_on_crafted_frames(oracle, monkeypatch):
    """k_out behind the streaming k_fc at an odd width: output rows 12 bytes apart, P = 3 (mod 4)"""
    _case(KIND_ES, 3, 131, ("k_conv12", None, "k_fc"), {}, monkeypatch)


@pytest.mark.parametrize("n,wgs,fc", F.ACT_LARGE_ROWS, ids=[str(r[0]) for r in F.ACT_LARGE_ROWS])
def test_large_model_act_routes_on_crafted_frames(n, wgs, fc, oracle, monkeypatch):
    _case(KIND_GA_LARGE, NACT, n, ("lconv", (wgs, wgs), fc), {}, monkeypatch)
