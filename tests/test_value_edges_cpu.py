"""CPU: the premises of tests/test_gpu_value_edges.py, from the oracle alone (no engine, no GPU).

tests/value_edge_support.py multiplies one tensor group of a base vector by a power of two so that the layer behind it lands on FLT_MIN
(classes U1..U4) or on FLT_MAX (O1..O4, BIG).  Held here:

  * every class does what it is for: an under class's scaled layer has at least 10 % non-zero subnormal and at least 10 % normal outputs
    over the population at T = 1, an over class's at least 8 non-finite outputs and at least half finite ones;
  * O1 sends NaN through relu: the oracle's y2 holds NaN; without batch norm (GA) y3 is all NaN and the logits are the out bias exactly;
  * the oracle neither flushes nor reorders: sampled conv1 outputs (U1, O1) and fc columns (U3, O3) equal, bit for bit, an fmaf chain in
    the written order restated with dense_support.fmaf32 (correctly rounded at both ends of the range) -- the plain reference the GPU
    comparison rests on, and a check that this host does not run with flush-to-zero set;
  * step_tap_support.activated_y2 equals bn_relu of oracle/dne_oracle.c on NaN, +-inf, +-0, a subnormal and a NaN scale.

Wall time of the whole file: DESIGN.md section 3, "the contract's domain"."""
import numpy as np
import pytest

import oracle as O
import step_tap_support as S
import value_edge_support as V
from dense_support import fmaf32
from value_edge_support import KIND_ES, KIND_ES_VBN, KIND_GA, KIND_GA_LARGE

_KIND_IDS = {KIND_ES: "es", KIND_ES_VBN: "vbn", KIND_GA: "ga", KIND_GA_LARGE: "large"}
_CASES = [pytest.param(k, c, id="%s-%s" % (_KIND_IDS[k], c)) for k in (KIND_ES, KIND_ES_VBN, KIND_GA, KIND_GA_LARGE) for c in V.CLASSES[k]]


def _scaled_outputs(kind, cls):
    """the scaled layer's output of every member at T = 1, concatenated"""
    if kind == KIND_GA_LARGE:
        taps, k = [V.large_taps(cls, m)[1] for m in range(V.N_LARGE)], V.LARGE_SCALED_OUTPUT[cls]
    else:
        taps, k = [V.taps(kind, cls, m)[1] for m in range(2 * V.N_PAIRS)], V.SCALED_OUTPUT[cls]
    assert all(t["length"] == 1 for t in taps)
    return np.concatenate([(list(t["y"]) + [t["logits"]])[k] for t in taps])


@pytest.mark.parametrize("kind,cls", _CASES)
def test_class_mix(kind, cls):
    c = V.census(_scaled_outputs(kind, cls))
    print(_KIND_IDS[kind], cls, V.CLASSES[kind][cls], c)
    if V.is_under(cls):
        assert c["subnormal"] >= 0.1 * c["size"] and c["normal"] >= 0.1 * c["size"], c
        assert c["inf"] == 0 and c["nan"] == 0, c
        s = np.float32(V.sigma_of(kind, cls))
        assert 0 < s < V.FLT_MIN                     # fl(sigma * eps) is subnormal wherever |eps| < 1: most of the table
    else:
        assert c["inf"] + c["nan"] >= 8 and c["normal"] + c["subnormal"] + c["zero"] >= 0.5 * c["size"], c


def test_ga_base_is_the_scaled_normc_start():
    """a GA engine forms the parent itself, as noise * scale_by: with the normc factors as scale_by that is oracle.ga_rebuild's vector (a zeroed
    bias as +-0), and with a class's groups times 2^e it is that vector with the groups times 2^e"""
    start = O.ga_rebuild(O.layout(O.KIND_GA, S.NACT), S.small_noise(), list(V.GA_PARENT), V.GA_SIGMA)
    with np.errstate(all="ignore"):
        assert np.array_equal(S.small_noise()[V.GA_PARENT[0]:V.GA_PARENT[0] + S.P_GA] * V._normc_scale_by(), start)
    x = np.abs(S.small_noise()[V.GA_PARENT[0]:V.GA_PARENT[0] + S.P_GA]).max()
    for cls in V.CLASSES[KIND_GA]:
        got, want = V.base(KIND_GA, cls).astype(np.float64), V.scale_groups(start, KIND_GA, cls).astype(np.float64)
        # in an under class the factor times 2^e is itself subnormal: half a step of 2^-149 from its rounding, times |noise|, half a step
        # from the product's rounding, and on the other side half a step each from the start's rounding (scaled) and from the scaling
        steps = 0.5 * float(x) + 1.5 if V.is_under(cls) else 0.0
        assert np.abs(got - want).max() <= steps * 2.0 ** -149, cls
        assert len(V.ga_genomes(cls)) == V.GA_EVAL_MEMBERS


@pytest.mark.parametrize("kind", [KIND_ES, KIND_ES_VBN], ids=["es", "vbn"])
def test_u1_reaches_the_batch_moments(kind):
    """under U1 the batch means of conv1's 16 channels are subnormal (its variances underflow to 0): ModelVirtualBN's batch-norm shifts
    absorb a flushed y1 everywhere behind bn1, so for that kind the moments are what the GPU comparison of a fused conv1 rests on"""
    for m in range(2 * V.N_PAIRS):
        c = V.census(V.moments(kind, "U1", m)[:16])
        assert c["subnormal"] >= 8 and c["nan"] == 0 and c["inf"] == 0, (kind, m, c)


def test_no_episode_ends_by_the_last_tap():
    for kind in (KIND_ES, KIND_ES_VBN, KIND_GA):
        for cls in V.CLASSES[kind]:
            for m in range(2 * V.N_PAIRS):
                assert all(V.taps(kind, cls, m)[T]["length"] == T for T in V.TAPS), (kind, cls, m)


@pytest.mark.parametrize("kind", [KIND_ES, KIND_ES_VBN, KIND_GA], ids=["es", "vbn", "ga"])
def test_o1_sends_nan_through_relu(kind):
    for m in range(2 * V.N_PAIRS):
        tap = V.taps(kind, "O1", m)[1]
        y1, y2, y3 = tap["y"]
        assert np.isinf(y1).any() and not np.isnan(y1).any() and np.isnan(y2).any(), (kind, m)
        if kind == KIND_GA:                          # no batch norm: every fc chain meets a NaN, relu sends each to +0, 0 * w + bias
            L = O.layout(O.KIND_GA, S.NACT)
            assert np.isnan(y3).all()
            assert np.array_equal(tap["logits"].view(np.int32), V.member_theta(kind, "O1", m)[L.ob:L.ob + S.NACT].view(np.int32)), (kind, m)
        else:                                        # the NaN reaches the batch-norm statistics of the reference pass
            assert np.isnan(tap["bn"]).any(), (kind, m)


# ---- the oracle against an fmaf32 restatement of its written order ------------------------------------------------------------------------------
def _conv1_positions():
    """32 (oy, ox): the four corners, two border positions per side, the rest seeded"""
    rs = np.random.RandomState(32)
    pos = [(0, 0), (0, 20), (20, 0), (20, 20), (0, 7), (0, 13), (20, 7), (20, 13), (7, 0), (13, 0), (7, 20), (13, 20)]
    while len(pos) < 32:
        p = (int(rs.randint(0, 21)), int(rs.randint(0, 21)))
        if p not in pos:
            pos.append(p)
    return pos


def _conv1_restated(w, b, ob, oy, ox):
    """conv1_raw_acc of oracle/dne_oracle.c at one position, all 16 channels: an fmaf chain in (kh, kw, ci) order from +0 over the taps
    inside the image on float32(u8) / 255, then + bias"""
    lut = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    acc = np.zeros(16, np.float32)
    for kh in range(8):
        iy = oy * 4 - 2 + kh
        if not 0 <= iy < 84:
            continue
        for kw in range(8):
            ix = ox * 4 - 2 + kw
            if not 0 <= ix < 84:
                continue
            for ci in range(4):
                with np.errstate(all="ignore"):
                    acc = fmaf32(np.full(16, lut[ob[iy, ix, ci]], np.float32), w[kh, kw, ci], acc)
    with np.errstate(all="ignore"):
        return (acc + b).astype(np.float32)


@pytest.mark.parametrize("kind", [KIND_ES, KIND_GA], ids=["es", "ga"])
@pytest.mark.parametrize("cls", ["U1", "O1"])
def test_oracle_conv1_is_the_written_fmaf_chain(kind, cls):
    L = O.layout(O.KIND_GA if kind == KIND_GA else O.KIND_ES, S.NACT)
    th = V.member_theta(kind, cls, 0)
    ob = O.WrappedEnv().reset(int(V.SEEDS[0]))
    y1 = V.taps(kind, cls, 0)[1]["y"][0].reshape(21, 21, 16)
    w, b = th[L.c1w:L.c1w + 4096].reshape(8, 8, 4, 16), th[L.c1b:L.c1b + 16]
    seen = []
    for oy, ox in _conv1_positions():
        want = _conv1_restated(w, b, ob, oy, ox)
        assert V.bits_differ(y1[oy, ox], want) is None, (kind, cls, oy, ox, y1[oy, ox], want)
        seen.append(want)
    c = V.census(np.concatenate(seen))
    assert (c["subnormal"] > 0 and c["normal"] > 0) if cls == "U1" else c["normal"] > 0, c     # the sample itself straddles the edge


_FC_SUB = (0, 128, 248, 368, 488, 608, 728, 848, 968)     # ORC_FC_SUB: the sub-slice boundaries within a quarter (forward.h's header)
_FC_COLUMNS = (0, 1, 63, 64, 127, 200, 254, 255)


def _fc_restated(w, b, a2, cols):
    """fc_raw of oracle/dne_oracle.c on some columns: per quarter of 968 rows the left fold of 8 sub-slice fmaf chains (each from +0),
    then ((q0 + q1) + (q2 + q3)) + bias"""
    cols = list(cols)
    quarters = []
    with np.errstate(all="ignore"):
        for q in range(4):
            Q = None
            for i in range(8):
                u = np.zeros(len(cols), np.float32)
                for k in range(q * 968 + _FC_SUB[i], q * 968 + _FC_SUB[i + 1]):
                    u = fmaf32(np.full(len(cols), a2[k], np.float32), w[k, cols], u)
                Q = u if Q is None else (Q + u).astype(np.float32)
            quarters.append(Q)
        t = ((quarters[0] + quarters[1]).astype(np.float32) + (quarters[2] + quarters[3]).astype(np.float32)).astype(np.float32)
        return (t + b[cols]).astype(np.float32)


@pytest.mark.parametrize("kind", [KIND_ES, KIND_GA], ids=["es", "ga"])
@pytest.mark.parametrize("cls", ["U3", "O3"])
def test_oracle_fc_is_the_written_sub_slice_fold(kind, cls):
    L = O.layout(O.KIND_GA if kind == KIND_GA else O.KIND_ES, S.NACT)
    th = V.member_theta(kind, cls, 0)
    tap = V.taps(kind, cls, 0)[1]
    _, y2, y3 = tap["y"]
    a2 = S.activated_y2(y2, tap["bn"]) if kind == KIND_ES else np.where(y2 > 0, y2, np.float32(0.0)).astype(np.float32)
    want = _fc_restated(th[L.fcw:L.fcw + 3872 * 256].reshape(3872, 256), th[L.fcb:L.fcb + 256], a2, _FC_COLUMNS)
    assert V.bits_differ(y3[list(_FC_COLUMNS)], want) is None, (kind, cls, y3[list(_FC_COLUMNS)], want)


# ---- activated_y2 against bn_relu --------------------------------------------------------------------------------------------------------
def _bn_relu(x, scale, shift):
    """bn_relu of oracle/dne_oracle.c, statement by statement on float32 scalars"""
    with np.errstate(all="ignore"):
        t = np.float32(np.float32(x) * np.float32(scale))
        t = np.float32(t + np.float32(shift))
    return t if t > np.float32(0.0) else np.float32(0.0)


def test_activated_y2_is_the_oracles_select():
    sub = np.float32(2.0 ** -140)
    vals = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, sub, -sub, 1.5, -1.5, 3e38, -3e38], np.float32)
    y2 = np.resize(vals, 3872).astype(np.float32)
    rs = np.random.RandomState(7)
    bn = rs.randn(O.BN_FLOATS).astype(np.float32)
    bn[32 + 3] = np.nan                              # a NaN scale, a NaN shift, scales of 0, -0 and -1 (x * scale = -0 from +0 inputs), a zero shift
    bn[64 + 5] = np.nan
    bn[32 + 7], bn[64 + 7] = 0.0, 0.0
    bn[32 + 9], bn[64 + 9] = -0.0, 0.0
    bn[32 + 11], bn[64 + 11] = -1.0, -0.0
    bn[32 + 13], bn[64 + 13] = 1.0, 0.0
    bn[32 + 15], bn[64 + 15] = 3.0, np.inf           # inf * 3 + inf, -inf * 3 + inf = NaN
    got = S.activated_y2(y2, bn)
    want = np.array([_bn_relu(y2[i], bn[32 + (i & 31)], bn[64 + (i & 31)]) for i in range(y2.size)], np.float32)
    assert got.dtype == np.float32 and not np.isnan(want).any()          # relu's select lets no NaN through
    assert np.array_equal(got.view(np.int32), want.view(np.int32))      # bit patterns: no -0 either
    assert (want.view(np.int32) >= 0).all() and np.isinf(want).any() and (want == 0).any()
