"""The GA genome store on the device, generation after generation: which vector every member is evaluated on (all P floats, against the
oracle's rebuild and a float64 bound), its episode, and the discipline of the base slots -- tests/ga_store_support.py has the scenarios and
check_generation, tests/test_ga_store_cpu.py runs the same scenarios on a Python model of the store.  Knobs are read at dne_create, so every
case builds its own engine under its own environment."""
import numpy as np
import pytest

import ga_store_support as G
from ga_store_support import KIND_GA, KIND_GA_LARGE

pytestmark = pytest.mark.gpu

FORMS = ("sigma", "powers")
MATERIALIZE = ("0", "1")


@pytest.fixture
def make(monkeypatch, request):
    """make(kind) -> a fresh engine of MAX_MEMBERS members with its noise table, closed after the test; `knobs` marks set the environment"""
    from dne_hip import _lib
    made = []

    def _make(kind):
        e = _lib.Engine(kind, G.NACT, max_members=G.MAX_MEMBERS, record_bc=True)
        made.append(e)
        e.noise_upload(G.noise_of(kind))
        return e

    yield _make
    for e in made:
        e.close()


def knobs(monkeypatch, materialize, sort="1"):
    monkeypatch.setenv("DNE_GA_MATERIALIZE", materialize)
    monkeypatch.setenv("DNE_GA_SORT", sort)
    assert G.knobs_of(KIND_GA) == (int(materialize), int(sort))


@pytest.mark.parametrize("sort", ("0", "1"))
@pytest.mark.parametrize("materialize", MATERIALIZE)
@pytest.mark.parametrize("form", FORMS)
def test_eight_generations(make, monkeypatch, form, materialize, sort):
    knobs(monkeypatch, materialize, sort)
    G.scenario_generations(make, form)


@pytest.mark.parametrize("materialize", MATERIALIZE)
def test_large_model_generations_around_an_es_step(make, monkeypatch, materialize):
    knobs(monkeypatch, materialize)
    G.scenario_large_generations(make)


@pytest.mark.parametrize("materialize", MATERIALIZE)
@pytest.mark.parametrize("form", FORMS)
def test_prefix_starts_and_the_eight_seed_block(make, monkeypatch, form, materialize):
    knobs(monkeypatch, materialize)
    G.scenario_blocks(make, form)


@pytest.mark.parametrize("form", FORMS)
def test_chain_buffers_regrow(make, monkeypatch, form):
    knobs(monkeypatch, "0")
    G.scenario_regrow(make, form)


@pytest.mark.parametrize("materialize", MATERIALIZE)
def test_sigma_changes_between_calls(make, monkeypatch, materialize):
    knobs(monkeypatch, materialize)
    G.scenario_sigmas(make)


@pytest.mark.parametrize("materialize", MATERIALIZE)
def test_genome_form_switches_and_power_bits(make, monkeypatch, materialize):
    knobs(monkeypatch, materialize)
    G.scenario_forms(make)


@pytest.mark.parametrize("materialize", MATERIALIZE)
@pytest.mark.parametrize("form", FORMS)
def test_caller_owned_slots(make, monkeypatch, form, materialize):
    """On the engine as it was before dne_set_theta / dne_ga_rebuild* claimed the slot for the caller, all four cases failed at the warm-cache
    evaluation behind the rebuilds: the cache still mapped a parent to a slot the caller had overwritten, and its children were evaluated on the
    caller's chain -- "member 0 (engine row 0, slot 2) (14964,): 1008450 of 1008450 elements are not the oracle's" (sigma; powers the same with
    slot 2 / slot 4).  The mirror case below failed there too: "member 3 (engine row 4, slot 3) ...: evaluated out of slot 0 or a slot the
    caller wrote" without DNE_GA_MATERIALIZE, "slot 3, written by the caller, lost 1008450 of 1008450 elements" with it."""
    knobs(monkeypatch, materialize)
    G.scenario_caller_slots(make, form)


@pytest.mark.parametrize("materialize", MATERIALIZE)
@pytest.mark.parametrize("form", FORMS)
def test_caller_slot_written_before_the_first_generation(make, monkeypatch, form, materialize):
    knobs(monkeypatch, materialize)
    G.scenario_caller_slot_first(make, form)


@pytest.mark.parametrize("materialize", MATERIALIZE)
@pytest.mark.parametrize("form", FORMS)
def test_growth_and_shrinkage(make, monkeypatch, form, materialize):
    knobs(monkeypatch, materialize)
    G.scenario_growth(make, form)


@pytest.mark.parametrize("materialize", MATERIALIZE)
@pytest.mark.parametrize("form", FORMS)
def test_duplicates_and_elites(make, monkeypatch, form, materialize):
    knobs(monkeypatch, materialize)
    G.scenario_duplicates(make, form)


@pytest.mark.parametrize("materialize", MATERIALIZE)
@pytest.mark.parametrize("form", FORMS)
def test_refusals_leave_the_store_usable(make, monkeypatch, form, materialize):
    knobs(monkeypatch, materialize)
    G.scenario_refusals(make, form)


def test_debug_members_follows_set_members_and_es_eval(make):
    """the export outside the GA: identity order after set_members and es_eval, the table as uploaded, a short buffer is not overrun"""
    import ctypes as C
    e = make(KIND_GA_LARGE)
    assert [a.size for a in e.debug_members()] == [0, 0, 0, 0]
    e.set_theta(G.noise_of(KIND_GA_LARGE)[:e.P])
    e.set_theta(G.noise_of(KIND_GA_LARGE)[5:5 + e.P], slot=2)
    slot, off, scale = np.array([2, 0, 2], np.int32), np.array([7, G.last_offset(KIND_GA_LARGE), 0], np.int64), np.array([0.5, 0.0, -0.25], np.float32)
    e.set_members(slot, off, scale)
    got = e.debug_members()
    assert all(np.array_equal(a, b) for a, b in zip(got, (slot, off, scale, np.arange(3))))
    short = np.full(3, -7, np.int32)
    assert e.lib.dne_debug_members(e.h, 2, short.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None) == 3 and short.tolist() == [2, 0, -7]
    idx = np.array([11, 12], np.int64)
    e.es_eval(idx, 0.02, 2, np.arange(4, dtype=np.uint32))
    s2, o2, c2, w2 = e.debug_members()
    assert s2.tolist() == [0] * 4 and o2.tolist() == [11, 11, 12, 12] and w2.tolist() == [0, 1, 2, 3]
    assert np.array_equal(c2, np.array([0.02, -0.02, 0.02, -0.02], np.float32))
