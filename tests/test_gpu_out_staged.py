"""GPU: k_out's staged output layer -- whole-line loads of the [256][A] weight block, turned through LDS rows of A + 1 words -- at every
width the kernel is built for, against the CPU oracle value for value (y3, logits, actions; no tolerances).

dne_create admits 2..18 actions (the fixture's emulator has 18), so inside an engine only the 18-wide instantiation runs; there the head is
held by tests/test_gpu_step_taps.py (18 actions: ring, duo, sub_out, the GA forms), tests/test_gpu_action_widths.py (3, 4, 9, 17) and
tests/test_gpu_knife_edge.py, none of which this file repeats.  What an engine cannot reach is driven through dne_debug_out_head, which
launches k_out exactly as launch_fc does (launch_out) on arrays laid out here:

  widths    1 (one product per lane, a row of 2 words), 4, 17 and 18 (the 18-wide loops, full and one short: odd width = even row length),
            19 and 32 (the 32-wide loops; at 32 a pair stages 66 KB, above the 64 KB of DNE_OUT_LDS_KB)
  offsets   slices starting at every residue mod 4 floats, and one that ends at the table's last float
  kinds     groups of one (k_out<1, ..>) and antithetic pairs (k_out<2, ..>), each with batch norm (ES layout) and without (GA layout)
  lists     the null list; a compacted list, out of order, holding one group with one finished member and one with both finished,
            under the largest LDS reservation (64 KB), on the 32 chain sums of k_fc_sub instead of the 4 quarter sums

The oracle has no head of its own to call: a member's y3 and logits come from orc_forward_debug on an observation.  The fc partial sums fed
to the kernel are that y3 in the first slot and +0 in the others, over a flat vector and a noise table whose fc-bias entries are zero for every
member, so that ((q0 + q1) + (q2 + q3)) + bias -- arithmetic this file does not aim at -- returns the oracle's y3 exactly; everything behind
it (bn3 + relu, the weights fl(theta + fl(sc * eps)), 256 products per action, the lane tree, ((S0 + S1) + (S2 + S3)) + bias, first-max
argmax) is the oracle's against the kernel's.  Sentinels show what the kernel must leave alone: groups outside the list, finished groups,
the y3 row of a pair's finished member."""
import functools

import numpy as np
import pytest

import step_tap_support as S
from step_tap_support import KIND_ES, KIND_GA

pytestmark = pytest.mark.gpu

WIDTHS = (1, 4, 17, 18, 19, 32)
GROUPS = 6
SENT_F, SENT_A = np.float32(7.0), np.int32(-7)


def _table_len(P):
    return P + 4099


def _group_offsets(P):
    """residues 0, 1, 2, 3 mod 4 floats; the slice that ends at the table's last float; a 2 KB-aligned one"""
    off = np.array([0, 1, 1026, 2051, _table_len(P) - P, 512], np.int64)
    assert sorted(off[:4] % 4) == [0, 1, 2, 3] and off[4] + P == _table_len(P)
    return off


@functools.lru_cache(maxsize=None)
def _case(kind, gsize, nact):
    """inputs of one (kind, group size, width) and the oracle's y3 / logits / action per member, computed once"""
    import oracle as O
    L = O.layout(O.KIND_ES if kind == KIND_ES else O.KIND_GA, nact)
    P = L.P
    rs = np.random.RandomState(1000 * kind + 100 * gsize + nact)
    n = GROUPS * gsize
    goff = _group_offsets(P)
    off = np.repeat(goff, gsize)
    if gsize == 2:
        scale = np.tile(np.array([0.02, -0.02], np.float32), GROUPS)
    else:
        scale = np.array([0.02, -0.02, 0.0, 0.5, -0.1, 0.05], np.float32)
    base = (rs.randn(P) * 0.02).astype(np.float32)
    base[L.ow:L.ow + 256 * nact] *= np.float32(4.0)                  # logits well apart from their bias
    base[L.fcb:L.fcb + 256] = 0.0
    noise = rs.randn(_table_len(P)).astype(np.float32)
    for o in goff:
        noise[o + L.fcb:o + L.fcb + 256] = 0.0                        # every member's fc bias is +0 (module docstring)
    bn = None
    if kind == KIND_ES:
        bn = np.concatenate([rs.uniform(0.5, 1.5, (n, 16)), rs.randn(n, 16) * 0.1, rs.uniform(0.5, 1.5, (n, 32)), rs.randn(n, 32) * 0.1,
                             rs.uniform(0.5, 1.5, (n, 256)), rs.randn(n, 256) * 0.1], axis=1).astype(np.float32)
        assert bn.shape == (n, 608)
    obs = rs.randint(0, 256, (n, 84, 84, 4)).astype(np.uint8)
    y3 = np.empty((n, 256), np.float32); lg = np.empty((n, nact), np.float32); act = np.empty(n, np.int32)
    for m in range(n):
        th = (base + (np.float32(scale[m]) * noise[off[m]:off[m] + P]).astype(np.float32)).astype(np.float32)
        assert not th[L.fcb:L.fcb + 256].any()
        _, _, y3[m], lg[m] = O.forward_debug(L, th, None if bn is None else bn[m], obs[m])
        act[m] = S.argmax_first(lg[m])
    relu_in = y3 if bn is None else y3 * bn[:, 96:352] + bn[:, 352:608]
    assert ((relu_in > 0).sum(axis=1) > 16).all() and np.isfinite(lg).all()   # live inputs: the logits are sums of real products
    for a in (noise, base, off, scale, y3, lg, act):
        a.setflags(write=False)
    return dict(L=L, noise=noise, base=base, off=off, scale=scale, bn=bn, y3=y3, lg=lg, act=act)


def _sums(y3, sub):
    s = np.zeros((y3.shape[0], 32 if sub else 4, 256), np.float32)
    s[:, 0] = y3
    return s


def _run(kind, gsize, nact, c, **kw):
    from dne_hip import _lib
    n = c["off"].size
    y3 = np.full((n, 256), SENT_F, np.float32); act = np.full(n, SENT_A, np.int32); lg = np.full((n, nact), SENT_F, np.float32)
    _lib.debug_out_head(kind, gsize, nact, c["noise"], c["base"], c["off"], c["scale"], _sums(c["y3"], kw.get("sub_sums", False)), y3, act, lg,
                        bn=c["bn"], **kw)
    return y3, act, lg


def _ulp(got, want):
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    return "%d of %d differ, first at %s: %r vs %r" % (bad.size, got.size, bad[:4].tolist(), got.flat[bad[0]], want.flat[bad[0]]) if bad.size else "equal"


@pytest.mark.parametrize("nact", WIDTHS)
@pytest.mark.parametrize("gsize", [1, 2], ids=["single", "pair"])
@pytest.mark.parametrize("kind", [KIND_ES, KIND_GA], ids=["bn", "plain"])
def test_null_list(kind, gsize, nact):
    """every group, nobody finished, no reservation: y3, logits and actions of every member"""
    c = _case(kind, gsize, nact)
    y3, act, lg = _run(kind, gsize, nact, c)
    for m in range(c["off"].size):
        assert np.array_equal(y3[m], c["y3"][m]), (m, "y3", _ulp(y3[m], c["y3"][m]))
        assert np.array_equal(lg[m], c["lg"][m]), (m, int(c["off"][m]), "logits", _ulp(lg[m], c["lg"][m]), lg[m].tolist(), c["lg"][m].tolist())
        assert act[m] == c["act"][m] and 0 <= act[m] < nact, (m, act[m], c["act"][m])


@pytest.mark.parametrize("nact", WIDTHS)
@pytest.mark.parametrize("gsize", [1, 2], ids=["single", "pair"])
@pytest.mark.parametrize("kind", [KIND_ES, KIND_GA], ids=["bn", "plain"])
def test_compacted_list_with_finished_members(kind, gsize, nact):
    """list = groups 4, 1, 5, 2 (4: the slice at the table's end); group 5 has one finished member (a pair's second; a single: itself), group
    2 is finished altogether; groups 0 and 3 are not in the list.  Chain sums of k_fc_sub, a 64 KB reservation."""
    c = _case(kind, gsize, nact)
    n = c["off"].size
    lst = np.array([4, 1, 5, 2], np.int32)
    done = np.zeros(n, np.int32)
    done[5 * gsize + gsize - 1] = 1
    done[2 * gsize:3 * gsize] = 1
    y3, act, lg = _run(kind, gsize, nact, c, list=lst, done=done, sub_sums=True, reserve_lds_kb=64)
    for g in range(GROUPS):
        ms = range(g * gsize, (g + 1) * gsize)
        live = g in lst and not all(done[m] for m in ms)
        for m in ms:
            if live and not done[m]:
                assert np.array_equal(y3[m], c["y3"][m]), (m, "y3", _ulp(y3[m], c["y3"][m]))
                assert np.array_equal(lg[m], c["lg"][m]), (m, "logits", _ulp(lg[m], c["lg"][m]))
                assert act[m] == c["act"][m], (m, act[m], c["act"][m])
            else:
                assert (y3[m] == SENT_F).all(), (m, "y3 row of a member that is finished or not listed was written")
            if not live:
                assert act[m] == SENT_A and (lg[m] == SENT_F).all(), (m, "a group that is finished or not listed was written")


@pytest.mark.parametrize("name", ["ring_product", "duo", "sub_out"])
def test_regimes_under_the_lds_reservation(name, monkeypatch):
    """inside an engine: k_out<2, true> behind k_fc_ring, k_fc_duo and k_fc_sub's chain sums on the 11 edge-index pairs with DNE_OUT_LDS_KB=64 --
    the request is then the reservation, not the kernel's 39 KB -- y2 / y3 rows, BN, returns and all 22 RAM trajectories (every step's action)"""
    from test_gpu_step_taps import _run_es_regime
    monkeypatch.setenv("DNE_OUT_LDS_KB", "64")
    _run_es_regime(KIND_ES, name, monkeypatch, 18, sigmas=(0.02,), check_ram=True)
