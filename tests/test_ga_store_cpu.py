"""The GA store's test support without a GPU: the reference vectors agree with each other, the float64 bound does not reject the oracle,
the scripted generations do to a parent cache what the GPU scenarios rely on, and check_generation -- run on a Python model of the store
(tests/ga_store_model.py) -- passes a correct store and notices each mistake the model can be built with."""
import numpy as np
import pytest

import ga_store_support as G
from ga_store_support import KIND_GA, KIND_GA_LARGE

# the chain lengths (seeds, root included) the issue names, and the longest the GPU scenarios build: 16 in the block scenario
# ([p, a, b] + 11 + the child's own), CHAIN_CAP + 8 + 3 mutations behind a root + the child's own in the regrow scenario
LENGTHS = (1, 2, 9, 12, 16, G.CHAIN_CAP + 8 + 3 + 2, 1040)


def test_lengths_cover_the_gpu_scenarios():
    used = set()
    for form in ("sigma", "powers"):
        for pop in G.scripted_generations(KIND_GA, form, 12, 3, 8) + list(G.block_chains(KIND_GA, form)) + list(G.growth_generations(form)):
            used |= {len(g) for g in pop}
        used |= {len(G.long_genome(KIND_GA, form, m + 1)) for m in (5, G.CHAIN_CAP + 8 + 3)}
    assert max(used - {G.CHAIN_CAP + 8 + 3 + 2}) <= 16 and max(used) == G.CHAIN_CAP + 8 + 3 + 2
    assert {1, 2, 9, 12, 16, max(used)} <= set(LENGTHS)


@pytest.mark.parametrize("form", ("sigma", "powers"))
@pytest.mark.parametrize("length", LENGTHS)
def test_restatements_agree_and_the_bound_holds_for_the_oracle(form, length):
    sb = G.scale_by(KIND_GA) if form == "powers" else None
    g = G.long_genome(KIND_GA, form, length - 1, seed=900)
    if length > 2:                              # the first and the last legal slice among the mutations
        g = g[:1] + (((0, -0.002) if form == "powers" else 0),) + g[2:-1] + (((G.last_offset(KIND_GA), 0.004) if form == "powers" else G.last_offset(KIND_GA)),)
    want = G.oracle_vector(KIND_GA, form, g, G.SIGMA, sb)
    assert np.array_equal(G.f32_chain(KIND_GA, form, g, G.SIGMA, sb), want)
    assert G.within_f64_bound(want, KIND_GA, form, g, G.SIGMA, sb) == 0
    if 1 < length <= 16:
        # ... and the bound is no formality: the same chain with its last mutation left out lies outside it nearly everywhere
        short = G.oracle_vector(KIND_GA, form, g[:-1], G.SIGMA, sb)
        assert G.within_f64_bound(short, KIND_GA, form, g, G.SIGMA, sb) > want.size // 2


def test_large_model_vectors_keep_the_bound():
    sb = G.scale_by(KIND_GA_LARGE)
    for pop in G.scripted_generations(KIND_GA_LARGE, "powers", 6, 2, 3)[1:]:
        g = pop[-1]
        want = G.oracle_vector(KIND_GA_LARGE, "powers", g, sb=sb)
        assert np.array_equal(G.f32_chain(KIND_GA_LARGE, "powers", g, sb=sb), want)
        assert G.within_f64_bound(want, KIND_GA_LARGE, "powers", g, sb=sb) == 0


def test_another_sigma_or_scale_is_another_vector():
    """what the sigma and the initial-scale scenarios tell apart differs in (nearly) every element"""
    g = G.scripted_generations(KIND_GA, "sigma", 8, 3, 3)[2][1]
    a, b = G.oracle_vector(KIND_GA, "sigma", g, 0.005), G.oracle_vector(KIND_GA, "sigma", g, 0.002)
    assert (a != b).mean() > 0.99
    pg = G.with_powers(g)
    a, b = (G.oracle_vector(KIND_GA, "powers", pg, sb=G.scale_by(KIND_GA, w)) for w in (0, 1))
    assert (a != b).mean() > 0.99
    up = G.power_bit_genomes(G.scripted_generations(KIND_GA, "sigma", 8, 3, 3)[2])
    v = [G.oracle_vector(KIND_GA, "powers", x, sb=G.scale_by(KIND_GA)) for x in up[:3]]
    assert (v[0] != v[1]).mean() > 0.1 and (v[0] != v[2]).mean() > 0.99      # one ulp of a power moves many elements, its sign nearly all


@pytest.mark.parametrize("form", ("sigma", "powers"))
def test_scripted_generations_exercise_the_store(form):
    gens = G.scripted_generations(KIND_GA, form, 12, 3, 8)
    assert gens == G.scripted_generations(KIND_GA, form, 12, 3, 8)              # a fixed RandomState
    assert [len(p) for p in gens] == [12] * 8 and [max(len(g) for g in p) for p in gens] == list(range(1, 9))
    hi = G.last_offset(KIND_GA)
    for pop in gens[1:]:
        assert {0, hi} <= {G.seeds_of(g)[-1] for g in pop}                      # first and last legal slice as mutations
    assert {0, hi} <= {g[0] for g in gens[0]}                                  # ... and as roots
    rows = G.store_model(gens, form)
    assert rows[0]["fresh"] == 12 and rows[1]["evicted"] >= 9
    assert sum(r["evicted"] for r in rows[2:]) >= 6                            # parents leave the cache in the later generations too
    assert sum(1 for r in rows for s in r["starts"] if s >= 2) >= 4            # k_chain_sum starts from a cached prefix of two or more seeds
    assert sum(1 for r in rows if r["elite_with_children"]) >= 3               # an elite next to its own children
    assert all(2 <= r["needed"] <= 4 for r in rows[1:])
    if form == "powers":
        assert {p for pop in gens for g in pop for _, p in g[1:]} == set(G.POWERS) and min(G.POWERS) < 0


def test_special_chains():
    for form in ("sigma", "powers"):
        call0, call1, call2 = G.block_chains(KIND_GA, form)
        rows = G.store_model([call0, call1, call2], form)
        assert sorted(rows[1]["starts"]) == [1, 1, 1] and sorted(rows[2]["starts"]) == [3, 3, 3] and rows[2]["needed"] == 4
        assert sorted(len(g) - 2 for g in call1[::2]) == [2, 8, 11] and sorted(len(g) - 4 for g in call2[:6:2]) == [2, 8, 11]
        small, big = G.growth_generations(form)
        assert (len(small), len(big)) == (4, 14)
        assert len({G.prefix_key(g, form) for g in small}) == 2 and len({G.prefix_key(g, form) for g in big}) == 7
        assert {G.prefix_key(g, form) for g in small} <= {G.prefix_key(g, form) for g in big}
        assert len({G.prefix_key(g, form) for g in G.four_parent_generation(form)}) == 4
    pw = [p for g in G.block_chains(KIND_GA, "powers")[1] for _, p in g[1:]]
    assert min(pw) < 0 and len(set(pw)) > 4
    assert len(G.long_genome(KIND_GA, "sigma", G.CHAIN_CAP + 8 + 3 + 1)) - 2 > G.CHAIN_CAP


# ---- check_generation and the scenarios on the model of the store ---------------------------------------------------------------------------
def model_maker(bug=None):
    import ga_store_model as M

    def make(kind):
        e = M.ModelStore(kind, max_members=G.MAX_MEMBERS, bug=bug)
        e.noise_upload(G.noise_of(kind))
        return e
    return make


def knobs(monkeypatch, materialize, sort="1"):
    monkeypatch.setenv("DNE_GA_MATERIALIZE", materialize)
    monkeypatch.setenv("DNE_GA_SORT", sort)
    assert G.knobs_of(KIND_GA) == (int(materialize), int(sort))


@pytest.mark.parametrize("materialize,sort", (("0", "0"), ("1", "1")))
def test_correct_model_passes_the_scenarios(monkeypatch, materialize, sort):
    knobs(monkeypatch, materialize, sort)
    make = model_maker()
    G.scenario_generations(make, "sigma", gens=4)
    G.scenario_blocks(make, "powers")
    G.scenario_sigmas(make)
    G.scenario_forms(make)
    G.scenario_caller_slots(make, "sigma")
    G.scenario_caller_slot_first(make, "powers")
    G.scenario_growth(make, "sigma")
    G.scenario_duplicates(make, "powers")
    G.scenario_refusals(make, "sigma")


@pytest.mark.parametrize("materialize", ("0", "1"))
@pytest.mark.parametrize("bug,scenario", (("sigma", "sigmas"), ("bits", "forms"), ("grow", "caller_slot_first"), ("stale", "caller_slots")))
def test_each_mistake_of_the_model_turns_its_scenario_red(monkeypatch, bug, scenario, materialize):
    knobs(monkeypatch, materialize)
    run = getattr(G, "scenario_" + scenario)
    args = () if scenario in ("sigmas", "forms") else ("sigma",)
    with pytest.raises(AssertionError):
        run(model_maker(bug), *args)
