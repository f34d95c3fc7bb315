"""CPU, oracle alone: the virtual-batch-norm statistics of the reference pass against float64 moments, degenerate batches included.

The engine's reference pass is compared with the oracle bit for bit, and the oracle's bn_finish_tiles was written to mirror the kernels, so
a mistake both share (a wrong count, a padded tile position that is not an exact zero, a bias counted twice, the clamp on the wrong side)
passes every such comparison.  Here the oracle's batch moments (es_ref_pass_moments) of every case of tests/vbn_stats_support.py -- a
perturbed start point, an ill-conditioned theta, all-zero / all-255 / repeated-frame batches, 254 / 255 noise under one-tap channels of
weight 3 .. 100, at 8, 16 and 128 reference frames, for the ES kind and for ModelVirtualBN (no biases, no gammas) -- are held against
float64 moments of the oracle's own layer outputs within tolerances derived in vbn_stats_support's docstring, and its scale / shift
against the contract of DESIGN.md section 3 bit for bit.  tests/test_gpu_vbn_stats.py runs the same assertion on the engine.

The check has teeth (the idea of tests/test_knife_edge_cpu.py): the moments restated in numpy float32 pass it, and each subtly wrong
restatement is reported by it.

The worst observed / tolerance ratio per layer is printed (pytest -s) and asserted below 1, nothing tighter; DESIGN.md section 3 records
the figures."""
import numpy as np
import pytest

import vbn_stats_support as V
from vbn_stats_support import CASES, FS, KINDS, LAYERS

RATIOS = {}      # (kind, case, F) -> check_statistics' ratios, filled by the first test and printed by the summary


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def _check(kind, case, F):
    oc = V.oracle_case(kind, case, F)
    if (kind, case, F) not in RATIOS:
        RATIOS[(kind, case, F)] = V.check_statistics(V.layout(), oc["theta"], F, oc["bn"], oc["mom"], oc["ref64"])
    return oc, RATIOS[(kind, case, F)]


@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_moments_within_float64_tolerances(kind, case, F):
    oc, ratios = _check(kind, case, F)
    print("%s case %s F=%d: " % (kind, case, F) + "  ".join("%s/%s %.4f" % (k + (v,)) for k, v in sorted(ratios.items())))
    assert all(r < 1 for r in ratios.values())
    L, th, mom = V.layout(), oc["theta"], oc["mom"]
    if case == "c":     # all-zero batch: conv1's pre-bias sums are exact zeros, so mean == bias and variance == 0 exactly, every channel
        assert np.array_equal(mom[0:16], th[L.c1b:L.c1b + 16]) and not mom[16:32].any()
        assert np.array_equal(oc["bn"][0:16], V.scale_shift32(mom[0:16], mom[16:32], th[L.bn1g:L.bn1g + 16], th[L.bn1b:L.bn1b + 16])[0])
    if case in "bcde":  # the all-zero channels: y = bias everywhere, a true zero variance
        for (name, c) in V.ILL["zero"]:
            o, C = {n: (o, C) for n, o, C, _ in LAYERS}[name]
            assert oc["ref64"][name][1][c] == 0, (name, c)
            if name != "fc":    # one pass over pre-bias sums that are exact zeros: exact.  (The fc layer's two passes sum F equal values, which
                assert mom[o + C + c] == 0, (name, c, mom[o + C + c])   # rounds: its variance there is delta^2-small, inside the tolerance, not 0)
                assert mom[o + c] == V.layer_params(L, th, name)[0][c], (name, c)
    if case == "f" and kind == "es":   # the clamp engaged by rounding: the oracle's variance exactly 0 where the float64 variance is positive
        c = V.F_CLAMP[F]
        assert mom[16 + c] == 0 and oc["ref64"]["conv1"][1][c] > 0
        raw = V.conv_moments32(oc["ys"][0], th[L.c1b:L.c1b + 16], True, clamp=False)[1]
        assert raw[c] < 0


def test_worst_ratio_per_layer():
    """the slack of the derived tolerances: worst observed error / tolerance over the cases, per kind, F and layer"""
    for kind in KINDS:
        for F in FS:
            worst = {}
            for case in CASES:
                for k, v in _check(kind, case, F)[1].items():
                    if v >= worst.get(k, (-1, None))[0]:
                        worst[k] = (v, case)
            print("%-3s F=%-3d " % (kind, F) + "  ".join("%s %s %.4f (%s)" % (k[0], k[1], v, c) for k, (v, c) in sorted(worst.items())))
            assert all(v < 1 for v, _ in worst.values())


def test_case_f_scale_of_the_one_tap_channels():
    """a documented property of the one-pass contract, not a failure: where mean^2 >> variance the fp32 variance carries an absolute
    error of ~1e-7 (mean^2 + var), which is inside the backward bound and still moves the scale (printed)"""
    L = V.layout()
    for F in FS:
        oc, _ = _check("es", "f", F)
        th = oc["theta"]
        var64 = oc["ref64"]["conv1"][1]
        sc64 = th[L.bn1g:L.bn1g + 16].astype(np.float64) / np.sqrt(var64 + 1e-3)
        rel = np.abs(oc["bn"][0:16] / sc64 - 1)
        m2 = (oc["ref64"]["conv1"][0] - th[L.c1b:L.c1b + 16]) ** 2
        for chans, what in ((V.F_DENSE, "dense"), (V.F_SPARSE, "sparse")):
            print("F=%-3d %-6s " % (F, what) + "  ".join("w=%g: m2 %.3g var64 %.3g var32 %.3g scale off %.2g"
                                                        % (w, m2[c], var64[c], oc["mom"][16 + c], rel[c]) for c, w in zip(chans, V.F_WEIGHTS)))
        assert np.isfinite(rel).all()
        # the fixture's frames are not such a batch: the scale agrees with float64 to 5 digits
        oa, _ = _check("es", "a", F)
        tha = oa["theta"]
        sa = tha[L.bn1g:L.bn1g + 16].astype(np.float64) / np.sqrt(oa["ref64"]["conv1"][1] + 1e-3)
        assert np.abs(oa["bn"][0:16] / sa - 1).max() < 1e-5


# ------------------------------------------------------------------------------------------------- the check has teeth
def _restated(oc, F, only=None, conv=None, fc=None, eps=V.EPS):
    """bn / moments [608] from the numpy fp32 restatement of the contract over the oracle's layer outputs; the switches of a wrong form go
    to layer `only` (None: all)"""
    L, th = V.layout(), oc["theta"]
    mom = np.empty(608, np.float32); bn = np.empty(608, np.float32)
    for (name, o, C, npos), y in zip(LAYERS, oc["ys"]):
        bias, beta, gam = V.layer_params(L, th, name)
        wrong = only in (None, name)
        if name == "fc":
            mean, var = V.fc_moments32(y, **((fc or {}) if wrong else {}))
        else:
            kw = (conv(name, F) if callable(conv) else (conv or {})) if wrong else {}
            mean, var = V.conv_moments32(y, bias, name == "conv1", **kw)
        mom[o:o + C] = mean; mom[o + C:o + 2 * C] = var
        bn[o:o + C], bn[o + C:o + 2 * C] = V.scale_shift32(mean, var, gam, beta, eps if wrong else V.EPS)
    return bn, mom


def _reported(kind, case, F, layer, **wrong):
    oc = V.oracle_case(kind, case, F)
    bn, mom = _restated(oc, F, only=layer, **wrong)
    try:
        V.check_statistics(V.layout(), oc["theta"], F, bn, mom, oc["ref64"], layers=(layer,))
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("kind", KINDS)
def test_restated_moments_pass(kind):
    """the contract's order restated in numpy float32 is accepted on every case (it is not the oracle's bit pattern everywhere: the fused
    multiply-adds are emulated through float64)"""
    for case in CASES:
        for F in FS:
            oc = V.oracle_case(kind, case, F)
            bn, mom = _restated(oc, F)
            V.check_statistics(V.layout(), oc["theta"], F, bn, mom, oc["ref64"])
            same = np.mean(mom.view(np.int32) == oc["mom"].view(np.int32))
            assert same > 0.9, (case, F, same)     # and it is the oracle's arithmetic up to those rare double roundings


def test_padded_positions_counted_is_reported():
    pad = lambda name, F: dict(count=F * {"conv1": 448, "conv2": 128}[name])
    for F in FS:
        for layer in ("conv1", "conv2"):
            assert _reported("es", "a", F, layer, conv=pad), (F, layer)
            assert _reported("vbn", "b", F, layer, conv=pad), (F, layer)


def test_unbiased_variance_is_reported_where_one_over_n_exceeds_the_bound():
    """n / (n - 1) moves the variance by var / (n - 1); the tolerance is about 2 gamma_{F+16} (var + 2 m^2).  At F = 8 (n = 3528 / 968 / 8)
    that is 2.8e-4 / 1e-3 / 0.14 of the variance against 2.9e-6 (var + 2 m^2): reported on every channel with m^2 < ~50 var.  At F = 128
    conv1 has n = 56448, 1 / (n - 1) = 1.77e-5 against 2 gamma_144 = 1.72e-5: below the bound on every channel with m^2 > 0.015 var, so
    conv1 cannot report it there; conv2 (n = 15488, 6.5e-5) still can on a channel with m^2 < 1.4 var, the fc layer (n = 128) always."""
    for layer in ("conv1", "conv2", "fc"):
        assert _reported("es", "a", 8, layer, conv=dict(unbiased=True), fc=dict(unbiased=True)), layer
    assert _reported("es", "a", 128, "fc", fc=dict(unbiased=True))
    for layer in ("conv1", "conv2"):
        print("F=128 %s unbiased variance reported: %s" % (layer, bool(_reported("es", "a", 128, layer, conv=dict(unbiased=True)))))


def test_bias_counted_twice_and_bias_left_out_are_reported():
    for F in FS:
        for layer in ("conv1", "conv2"):
            for case in ("a", "b"):
                assert _reported("es", case, F, layer, conv=dict(bias_in_sums=True)), (F, layer, case)
                assert _reported("es", case, F, layer, conv=dict(bias_in_mean=False)), (F, layer, case)


def test_missing_clamp_is_reported_where_rounding_engages_it():
    for F in FS:
        msg = _reported("es", "f", F, "conv1", conv=dict(clamp=False))
        assert msg and "negative variance" in msg, (F, msg)
        assert _reported("es", "f", F, "conv1") is None


def test_eps_1e_5_is_reported():
    for kind in KINDS:
        for case in CASES:
            for layer in ("conv1", "conv2", "fc"):
                assert _reported(kind, case, 16, layer, eps=np.float32(1e-5)), (kind, case, layer)


def test_dropped_last_tile_is_reported():
    for F in FS:
        for layer in ("conv1", "conv2"):
            assert _reported("es", "a", F, layer, conv=dict(drop_last_tile=True)), (F, layer)
            assert _reported("vbn", "a", F, layer, conv=dict(drop_last_tile=True)), (F, layer)


def test_dropped_frame_is_reported():
    for F in FS:
        for layer in ("conv1", "conv2", "fc"):
            for drop in (0, F - 1):
                assert _reported("es", "a", F, layer, conv=dict(drop_frame=drop), fc=dict(drop_frame=drop)), (F, layer, drop)
