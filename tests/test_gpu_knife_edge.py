"""GPU: every policy head that runs inside an evaluation pinned to ONE ulp, exact ties included.

Inside an evaluation the head's arithmetic -- bn3 + relu, the 256 x A (LargeModel 512 x A) output layer summed tree64 per wave and
(S0+S1)+(S2+S3), the bias last, the first-maximum argmax, and the commit by the lane that owns the chosen action -- is written out in
head_body (k_tail_step, k_tail_select, k_tail_select_conv1), k_fc's step mode, k_out<NV, HAS_BN>, k_fc2 and k_lout, and committed in three
ways (tid 0 steps the emulator; thread 256 + best commits its own candidate; the speculative tail adopts candidate `best`).  The logits are
not tapped there, and the ordinary populations' closest decision is hundreds of ulps from flipping.

tests/knife_edge_support.py builds, from the oracle alone, populations on noise tables of their own and per tap step T two versions of the
table, `lo` and `hi`, that differ in one float32 per member by one unit in the last place -- the entry behind one output bias -- such that
the oracle's decision at step T flips between the member's top action a and another column b: on one table logit_a == logit_b bit for bit
(the first maximum decides), on the other they are adjacent floats.  A head that is off by one ulp on either logit, sums in another
order where that shows, takes the twin's bias, or breaks a tie the other way commits another action than the oracle on at least one of the
two tables, and every step's action is RAM byte 38 of the recorded trajectory (tests/test_knife_edge_cpu.py: the construction's
conditions, and six wrong heads each reported by the comparison used here).

Each case forces its regime with the knobs of tests/test_gpu_step_taps.py / tests/test_gpu_edges.py (imported, not copied) before
Engine(...), uploads the population's table once, and per T: noise_write the `lo` entries, evaluate, noise_write the `hi` entries, evaluate;
every member (knife-edge or not) is the oracle's on both tables -- every step's RAM row (GA kinds: the final RAM), return, sign-return,
length == T -- plus profile()["fc_full_kind"] where the regime defines it and check_redzones() == 0.  A failure names the regime, T, the
member, a, b, the table and whether that table held the tie or the one-ulp side.

On an MI355X the 69 default cases take 10 s and the 33 variants 4 s (0.04 to 0.1 s each after the session's first engine; the oracle side of
every population is built once per session and shared through knife_edge_support's cache)."""
import numpy as np
import pytest

import knife_edge_support as K
import step_tap_support as S
from step_tap_support import NACT, NREF, KIND_ES, KIND_ES_VBN
from test_gpu_edges import _VARIANT_KEYS
from test_gpu_step_taps import ES_REGIMES, VBN_REGIMES, _LARGE_CASES, _es_engine, _es_variant_params, _fc_full_kind, _ga_params

pytestmark = pytest.mark.gpu


class _Table:
    """the population's table on the engine, with the entries of one (case, "lo" | "hi") written over it"""

    def __init__(self, e, pop):
        self.e, self.pop, self.dirty = e, pop, np.zeros(0, np.int64)

    def set(self, c, which):
        for p in self.dirty:                                         # (the previous case's entries back to the table's own values)
            self.e.noise_write(int(p), self.pop.table[p:p + 1])
        for p, v in zip(c.pos, c.vals[which]):
            self.e.noise_write(int(p), np.array([v], np.float32))
        self.dirty = c.pos
        got = np.array([self.e.noise_get(int(p), 1)[0] for p in c.pos], np.float32)
        assert np.array_equal(got.view(np.int32), c.vals[which].view(np.int32)), (which, "the table on the device is not the case's")


def _run(pop, e, evaluate, ctx, fc_kind=None):
    """evaluate(T) -> (returns, sign-returns, lengths, RAM) of the whole population on the engine's current table"""
    table = _Table(e, pop)
    for T in pop.taps:
        c = K.case(pop, T)

        def run(which):
            table.set(c, which)
            out = evaluate(T)
            if fc_kind is not None:
                assert e.profile()["fc_full_kind"] == fc_kind, (ctx, T, which)   # the forced regime really ran (5 ring, 4 sub, 3 duo, 2 k_fc2, 1 k_fc / tail)
            return out

        K.compare(c, run, ctx)
    assert e.check_redzones() == 0


def _run_es(kind, knobs, fc_kind, profile, monkeypatch, ctx, nact=NACT):
    pop = K.es_population(kind, nact)
    e = _es_engine(kind, knobs, len(pop.idx), monkeypatch, profile, nact, record_ram=True, noise=pop.table)
    try:
        _run(pop, e, lambda T: e.es_eval(pop.idx, K.SIGMA, T, pop.seeds, want_bc=True), ctx, fc_kind)
    finally:
        e.close()


@pytest.mark.parametrize("name", list(ES_REGIMES))
def test_es_regime_heads(name, monkeypatch):
    """every row of test_gpu_step_taps.ES_REGIMES (its comment names the kernels) at sigma 0.02 on the 11 pairs, T = 1, 3, 9: k_out<2, true>
    behind the ring / duo, k_out<2, true> on the chain sums, k_tail_step behind k_fc_sub / k_fc_quad / k_fc_tail / k_fc_cols,
    k_tail_select_conv1 / k_tail_select in the speculative tail"""
    knobs, fc_kind, _, _ = ES_REGIMES[name]
    _run_es(KIND_ES, knobs, fc_kind, fc_kind is not None, monkeypatch, name)


@pytest.mark.parametrize("name", VBN_REGIMES)
def test_vbn_regime_heads(name, monkeypatch):
    """DNE_KIND_ES_VBN: the heads' opt_bias / no-conv-bias forms; the edited entry is the out/b position of the kind's own flat layout"""
    knobs, fc_kind, _, _ = ES_REGIMES[name]
    _run_es(KIND_ES_VBN, knobs, fc_kind, fc_kind is not None, monkeypatch, "vbn " + name)


@pytest.mark.parametrize("knobs", _es_variant_params())
def test_es_step_knob_heads(knobs, monkeypatch):
    """the entries of test_gpu_edges._ES_STEP_KNOBS that are no row of ES_REGIMES (variants by the rule of _knob_params): k_fc2's own head,
    k_fc<2>'s step mode (DNE_FC_PAIRS), DNE_HEAD_THREADS=256 (the head without its fifth wave: one lane steps the emulator),
    DNE_DUO_HEAD_FUSED, DNE_SUB_RENDER_FUSED, DNE_TAIL_FUSED_MAX=0 (k_out + separate emulator launch), DNE_TAIL_TABLE=0, ..."""
    _run_es(KIND_ES, knobs, _fc_full_kind(knobs), False, monkeypatch, ",".join("%s=%s" % kv for kv in knobs.items()))


@pytest.mark.parametrize("nact", [3, 17])
@pytest.mark.parametrize("name", ["ring_product", "tail_default", "tail_spec"])
def test_es_regime_heads_at_width(name, nact, monkeypatch):
    """widths 3 and 17 at T = 1: the `tid < nact` and NV * nact lane masks, the candidate count of the speculative tail and of the fifth
    wave are not 18's"""
    knobs, fc_kind, _, _ = ES_REGIMES[name]
    _run_es(KIND_ES, knobs, fc_kind, fc_kind is not None, monkeypatch, "%s at %d actions" % (name, nact), nact)


@pytest.mark.parametrize("knobs", [{}, {"DNE_SPEC_MAX": "64"}, {"DNE_FC_TAIL_MAX": "1"}], ids=["tail_default", "tail_spec", "k_fc"])
def test_mixed_scale_member_heads(knobs, monkeypatch):
    """set_members + eval_members, groups of one (scales 0.02, -0.02, 0, 0.5, -0.1 on windows of their own): k_tail_step behind
    k_fc_tail<1, true>, the speculative tail's k_tail_select[_conv1] behind k_fc_quad_spec<1, true>, and k_fc<1>'s step mode"""
    from dne_hip import _lib
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    pop = K.mixed_population()
    e = _lib.Engine(_lib.KIND_ES, NACT, max_members=8, ref_count=NREF, record_bc=True, bc_max_steps=max(pop.taps))
    try:
        e.noise_upload(pop.table); e.set_ref_batch(S.ref_batch()); e.set_theta(S.base_theta(KIND_ES))

        def evaluate(T):
            e.set_members(np.zeros(pop.n, np.int32), pop.off, pop.scale)
            return e.eval_members(pop.n, T, pop.seeds, want_bc=True)

        _run(pop, e, evaluate, ("mixed scales", knobs))
    finally:
        e.close()


@pytest.mark.parametrize("knobs", _ga_params())
def test_ga_regime_heads(knobs, monkeypatch):
    """KIND_GA (no batch norm, NV = 1): seven children, member by member (DNE_GA_SORT=0), T = 1 and 6, through the default path and every
    entry of test_gpu_edges._GA_STEP_KNOBS; the edited entry lies in the child's mutation window; the final RAM carries the last action"""
    from dne_hip import _lib
    for k, v in dict(knobs, DNE_GA_SORT="0").items():
        monkeypatch.setenv(k, v)
    pop = K.ga_population()
    e = _lib.Engine(_lib.KIND_GA, NACT, max_members=16, record_bc=True)
    try:
        e.noise_upload(pop.table)
        _run(pop, e, lambda T: e.ga_eval([list(c) for c in pop.chains], S.GA_SIGMA, T, pop.seeds, want_bc=True), ("ga", knobs))
    finally:
        e.close()


def _large_params():
    """the six-member rows of _LARGE_CASES; behind `variants` where a row carries a _VARIANT_KEYS knob (the rule of test_gpu_edges._knob_params)"""
    return [pytest.param(*p.values, id=p.id, marks=[pytest.mark.variants] if _VARIANT_KEYS & set(p.values[1]) else [])
            for p in _LARGE_CASES if p.values[0] == 6]


@pytest.mark.parametrize("n,knobs", _large_params())
def test_large_model_heads(n, knobs, monkeypatch):
    """KIND_GA_LARGE, k_lout (K = 512: eight group sums): a root and five children with powered mutations, T = 1 and 3, through the
    six-member cases of test_gpu_step_taps._LARGE_CASES"""
    from dne_hip import _lib
    for k, v in dict(knobs, DNE_GA_SORT="0").items():
        monkeypatch.setenv(k, v)
    pop = K.large_population()
    assert pop.n == n
    e = _lib.Engine(_lib.KIND_GA_LARGE, NACT, max_members=n, record_bc=True)
    try:
        e.noise_upload(pop.table)
        e.ga_set_init_scale(pop.scale_by)
        _run(pop, e, lambda T: e.ga_eval_powers(pop.genomes, T, pop.seeds, want_bc=True), ("large", knobs))
    finally:
        e.close()
