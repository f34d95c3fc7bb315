"""CPU: the knife-edge populations of tests/knife_edge_support.py are what tests/test_gpu_knife_edge.py takes them for, and the comparison
that file runs against the engine would fail on a subtly wrong policy head.

Construction: per (population, T) two tables that differ in one float32 per edited member, by one unit in the last place, between which the
ORACLE's step-T decision flips a <-> b with logit_a, logit_b bit-equal on one table and adjacent floats on the other.  The conditions below
are not measurements: the table seeds (knife_edge_support.TABLE_SEED) are chosen so that the oracle alone meets them; a seed that fails is
replaced, never the bar.  test_construction_conditions prints the counts per (kind, width, T) (pytest -s).

Sensitivity: knife_edge_support.compare() takes "an engine"; here it gets a CPU stand-in that replays the oracle's episode and recomputes
step T's decision from the oracle's y3 / bn with a deliberately wrong head.  `>=` in the argmax, one logit one ulp up or down, the products
summed as one serial chain, the bias added before the group sums, the twin's bias: every one is reported, the oracle's own head passes.

Wall time of this module: 34 s on the development host (one core; the whole CPU suite: 2 min 10 s), of which the sensitivity tests
18 s and the construction of all seven populations 13 s; the oracle side is built once per session and shared."""
import numpy as np
import pytest

import knife_edge_support as K
import step_tap_support as S
from step_tap_support import NACT, KIND_ES, KIND_ES_VBN, KIND_GA, KIND_GA_LARGE

POPS = {
    "es-18": lambda: K.es_population(KIND_ES, NACT),
    "vbn-18": lambda: K.es_population(KIND_ES_VBN, NACT),
    "es-3": lambda: K.es_population(KIND_ES, 3),
    "es-17": lambda: K.es_population(KIND_ES, 17),
    "ga-18": K.ga_population,
    "large-18": K.large_population,
    "mixed-18": K.mixed_population,
}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def test_float_keys_are_the_order_of_float32():
    xs = np.array([-3.5, -1e-30, -1e-45, -0.0, 0.0, 1e-45, 1e-30, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), 3e38], np.float32)
    ks = [K.key(x) for x in xs]
    assert ks == sorted(ks) and ks[3] == ks[4] == 0 and ks[5] == 1 and ks[2] == -1 and ks[8] - ks[7] == 1
    for x in xs:
        assert K.unkey(K.key(x)) == x and K.unkey(K.key(x) + 1) == np.nextafter(x, np.float32(np.inf))
    assert K.ulps(np.float32(1.0), xs[8]) == 1 and K.ulps(np.float32(-1e-45), np.float32(1e-45)) == 2


def test_numpy_head_is_out_raw_k(oracle):
    """head_logits on random data against the oracle's own output layer (through forward_debug on the tap populations it is asserted for
    every bisected member; here: K = 256 and 512, widths 3, 17, 18, and that the wrong heads are NOT the oracle's arithmetic)"""
    for pop in (POPS["es-18"](), POPS["es-3"](), POPS["es-17"](), POPS["large-18"](), POPS["ga-18"]()):
        for m in (0, pop.n - 1):
            tap = K._base_rollouts(pop)[m][max(pop.taps)]
            w, bias, a, _ = pop.head_inputs(pop.table, m, tap)
            assert w.shape == (512 if pop.large else 256, pop.nact) and (a >= 0).all() and (a > 0).sum() > 32
            assert np.array_equal(K.head_logits(w, bias, a).view(np.int32), tap["logits"].view(np.int32)), (pop.name, m)
    serial = (np.add.accumulate((a[:, None] * w).astype(np.float32), axis=0, dtype=np.float32)[-1] + bias).astype(np.float32)
    assert not np.array_equal(serial, K.head_logits(w, bias, a))     # (and head_serial really is another order)


def test_windows_are_disjoint_and_keep_the_alignment_classes():
    for kind, nact in ((KIND_ES, 18), (KIND_ES_VBN, 18), (KIND_ES, 3), (KIND_ES, 17)):
        P = S.num_params(kind, nact)
        idx, N = K.es_windows(P)
        s = np.sort(idx)
        assert len(idx) == 11 == len(S.edge_indices(P)) and (np.diff(s) >= P).all() and s[0] == 0 and s[-1] + P == N    # first / last legal slice
        assert {0, 1, 2, 3} <= {int(x) % 4 for x in idx} and any(x % 64 == 0 and x > 0 for x in idx) and any(x % 4 == 0 and x % 64 for x in idx)
        assert (np.diff(s) == P).sum() >= 2 and not np.array_equal(idx, s)                # windows that abut; member order is not table order
        pop = K.es_population(kind, nact)
        assert pop.table.size == N and pop.n == 22 and np.array_equal(pop.idx, idx) and N < 11.2e6
        assert np.array_equal(pop.seeds, S.tap_seeds(22)) and pop.theta(pop.table, 3).size == S.num_params(KIND_ES, nact)
    for pop, P, windows in ((K.ga_population(), S.P_GA, {x for c in K.ga_population().chains for x in c}),
                            (K.large_population(), S.num_params(KIND_GA_LARGE), {x if i == 0 else x[0] for g in K.large_population().genomes for i, x in enumerate(g)})):
        w = np.array(sorted(windows), np.int64)
        assert (np.diff(w) >= P).all() and w[0] == 0 and w[-1] + P == pop.table.size, pop.name
    assert len(K.ga_population().chains) == 7 and all(len(c) == 2 for c in K.ga_population().chains)          # children only
    assert sum(len(g) > 1 for g in K.large_population().genomes) >= 4 and K.large_population().n == 6
    mixed = K.mixed_population()
    assert (np.diff(np.sort(mixed.off)) >= S.P_ES).all() and (mixed.scale > 0).any() and (mixed.scale < 0).any() and (np.abs(mixed.scale) > K.SIGMA).any()


def _bars(pop, T, c):
    """the conditions a (kind, width, T) population must meet"""
    first = T == pop.taps[0]
    assert 3 * c["edges"] >= pop.n and (not first or 2 * c["edges"] >= pop.n), (pop.name, pop.nact, T, c)   # a third; at T = 1 half
    if pop.name == "mixed":        # five single members, one of them theta itself: an edge under a positive and under a negative scale, at T = 1 under one larger than sigma
        e = K.case(pop, T).edges()
        assert (pop.scale[e] > 0).any() and (pop.scale[e] < 0).any() and (not first or (np.abs(pop.scale[e]) > K.SIGMA).any()), (T, e)
        return
    assert c["b_below_a"] >= 2 and c["b_above_a"] >= 2, (pop.name, pop.nact, T, c)
    assert c["tie_on_lo"] >= 1 and c["tie_on_hi"] >= 1, (pop.name, pop.nact, T, c)


@pytest.mark.parametrize("name", list(POPS))
def test_construction_conditions(name):
    """at least half of the members are knife-edges at the first tap step and a third at every later one, two with b < a and two with
    b > a, the exact tie at least once on each table; widths 3 and 17: T = 1 only.  Also what the GPU test relies on: the tables differ
    from the population's in one float per edited member, inside that member's own window, lo and hi adjacent; every member's oracle
    episode is T steps long on both tables; a non-edge member keeps its place"""
    pop = POPS[name]()
    assert pop.taps == (S.TAP_STEPS if name in ("es-18", "vbn-18", "mixed-18") else S.GA_TAP_STEPS if name == "ga-18" else S.LARGE_TAP_STEPS
                        if name == "large-18" else (1,))
    for T in pop.taps:
        c = K.case(pop, T)
        counts = c.counts()
        print("knife-edges %-8s width %2d T %d: %2d of %2d members; b < a %2d, b > a %2d; tie on lo %2d, on hi %2d"
              % (pop.name, pop.nact, T, counts["edges"], pop.n, counts["b_below_a"], counts["b_above_a"], counts["tie_on_lo"], counts["tie_on_hi"]))
        _bars(pop, T, counts)
        assert len(c.members) == pop.n and len(set(c.pos.tolist())) == len(c.pos) <= pop.n
        assert all(K.ulps(x, y) == 1 and x < y for x, y in zip(c.vals["lo"], c.vals["hi"]))
        edited = [m for m in range(pop.n) if c.members[m]["a"] is not None]
        assert sorted(pop.entry0[m] + c.members[m]["b"] for m in edited) == sorted(c.pos.tolist())
        for which in ("lo", "hi"):
            tab = c.table(which)
            assert np.flatnonzero(tab != pop.table).size <= len(c.pos) and np.array_equal(tab[c.pos], c.vals[which])
            for m in range(pop.n):
                r = c.rollouts[which][m]
                assert r["length"] == T and r["actions"].shape == (T,) and np.array_equal(r["ram"][:, 38], r["actions"]), (name, T, m)
        for m in c.edges():
            d, lo, hi = c.members[m], c.rollouts["lo"][m], c.rollouts["hi"][m]
            assert d["a"] != d["b"] and np.array_equal(lo["actions"][:-1], hi["actions"][:-1])
            assert (lo["actions"][-1], hi["actions"][-1]) == ((d["a"], d["b"]) if pop.scale[m] > 0 else (d["b"], d["a"]))
            tie, other = c.rollouts[d["tie_on"]][m]["logits"], c.rollouts["hi" if d["tie_on"] == "lo" else "lo"][m]["logits"]
            assert tie[d["a"]].view(np.int32) == tie[d["b"]].view(np.int32) and K.ulps(other[d["a"]], other[d["b"]]) == 1
            assert S.argmax_first(tie) == min(d["a"], d["b"])                              # the first maximum takes the tie
            tw = pop.twin[m]
            if tw is not None:                                                             # the twin's episode never met the edited column
                assert d["b"] not in c.rollouts["lo"][tw]["actions"] and d["b"] not in c.rollouts["hi"][tw]["actions"] and c.members[tw]["b"] != d["b"]


def test_knife_edges_against_oracle_rollout(oracle):
    """the recorded episodes are oracle.rollout's on vectors built from the two final tables (ES, T = 3; step_tap_support's loop is pinned to
    oracle.rollout by tests/test_step_tap_cpu.py on the tap tests' table)"""
    pop = POPS["es-18"]()
    c = K.case(pop, 3)
    for which in ("lo", "hi"):
        tab = c.table(which)
        for m in c.edges()[:6]:
            th = oracle.perturb(S.base_theta(KIND_ES), tab, pop.idx[m // 2], K.SIGMA, 1 if m % 2 == 0 else -1)
            r = oracle.rollout(pop.L, th, pop.ref, pop.seeds[m], 3, want_bc=True, want_actions=True)
            want = c.rollouts[which][m]
            assert r[:3] == (want["ret"], want["sign"], 3) and np.array_equal(r[3], want["ram"]) and np.array_equal(r[4], want["actions"])


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------------
_SENS = [("es-18", 1), ("es-18", 3), ("es-18", 9), ("vbn-18", 1), ("es-3", 1), ("es-17", 1), ("ga-18", 1), ("ga-18", 6), ("large-18", 1), ("large-18", 3),
         ("mixed-18", 1)]


def _caught(c, head, ctx):
    with pytest.raises(AssertionError) as ei:
        K.compare(c, K.head_engine(c, head), ctx)
    msg = str(ei.value)
    assert ctx in msg and "T = %d" % c.T in msg and "member" in msg and "table '" in msg and ("exact tie" in msg or "one-ulp side" in msg), msg
    return msg


@pytest.mark.parametrize("name,T", _SENS)
def test_argmax_and_one_ulp_mutants_are_caught(name, T):
    """on every population and tap step: the oracle's head passes; an argmax with `>=` fails (on a member's tie table); one logit moved by
    +1 or -1 ulp fails for EVERY column that is the a or the b of a knife-edge member"""
    c = K.case(POPS[name](), T)
    K.compare(c, K.head_engine(c, K.head_oracle), name)
    msg = _caught(c, K.head_ge, name)
    assert "exact tie" in msg
    cols = sorted({c.members[m][k] for m in c.edges() for k in ("a", "b")})
    assert len(cols) >= 3
    for col in cols:
        for up in (True, False):
            _caught(c, K.head_ulp(col, up), name)


@pytest.mark.parametrize("name,T", [("es-18", 1), ("es-18", 3), ("es-18", 9), ("vbn-18", 1), ("es-17", 1), ("large-18", 1)])
def test_summation_order_mutants_are_caught(name, T):
    """the products summed as one serial chain instead of tree64 per wave, and the bias added before the group sums instead of last"""
    c = K.case(POPS[name](), T)
    _caught(c, K.head_serial, name)
    _caught(c, K.head_bias_first, name)


@pytest.mark.parametrize("name,T", [("es-18", 1), ("es-18", 3), ("es-18", 9), ("vbn-18", 1), ("es-3", 1), ("es-17", 1)])
def test_twin_bias_mutant_is_caught(name, T):
    """the bias taken from the pair's other member"""
    c = K.case(POPS[name](), T)
    _caught(c, K.head_twin_bias, name)
