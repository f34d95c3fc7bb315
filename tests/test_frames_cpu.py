"""CPU: the crafted frame set of tests/frames_support.py is what tests/test_gpu_frames.py needs it to be, and the harness that drives an engine
through a case (drive / check) is right before a GPU sees it -- run on the oracle behind the engine surface (tests/oracle_engine.py), it must
reproduce the oracle's own per-member values, and it must notice a frame, a member or a base slot that went to the wrong place."""
import numpy as np
import pytest

import frames_support as F
from frames_support import KIND_ES, KIND_ES_VBN, KIND_GA, KIND_GA_LARGE


def test_fixture_palette_is_what_design_md_records(oracle):
    """the measured palette of the rendered frames: 208 byte values, the absent list, channel-identical pixels, the most common value"""
    ref = F.fixture_batch()
    assert ref.shape == (128, 84, 84, 4) and ref.dtype == np.uint8
    absent = F.absent_values().tolist()
    assert len(np.unique(ref)) == 208 and len(absent) == 48
    assert absent == list(range(1, 5)) + [10, 11] + list(range(13, 31)) + [220, 225, 230, 233, 235] + list(range(237, 256))
    same = (ref == ref[..., :1]).all(axis=-1).mean()
    assert 0.80 < same < 0.82, same                                  # 81 % of pixels carry one value in all four stacked channels
    counts = np.bincount(ref.reshape(-1), minlength=256)
    assert int(np.argmax(counts)) == 63 and 0.18 < counts[63] / ref.size < 0.20


def test_frame_set_is_what_it_is_for(oracle):
    names, fr = F.frame_names(), F.frames()
    assert fr.shape == (22, 84, 84, 4) and fr.dtype == np.uint8 and len(set(names)) == len(names) == 22
    assert len({f.tobytes() for f in fr}) == 22
    by = dict(zip(names, fr))
    absent = F.absent_values()
    assert absent.size > 0 and 255 in absent
    seen = np.zeros(256, bool)
    seen[np.unique(F.fixture_batch())] = True
    for k in ("absent0", "absent1"):
        assert not seen[by[k]].any()                                 # no byte of the absent frames occurs in the 128 fixture frames
        assert set(np.unique(by[k]).tolist()) == set(absent.tolist())    # ... and every absent value is drawn
    assert not np.array_equal(by["absent0"], by["absent1"])
    ramp = by["ramp"]
    for c in range(4):
        assert len(np.unique(ramp[:, :, c])) == 256                  # all 256 values in every channel
    for a in range(4):
        for b in range(a + 1, 4):
            assert (ramp[:, :, a] != ramp[:, :, b]).all()            # the four channels differ at every pixel
    imp = [n for n in names if n.startswith("impulse")]
    assert len(imp) == len(F.IMPULSES) == 8
    for n, at in zip(imp, F.IMPULSES):
        assert np.count_nonzero(by[n]) == 1 and by[n][at] == 255
    planes = [by[n] for n in names if n.startswith("planes")]
    assert len(planes) == 3 and len({tuple(p[0, 0]) for p in planes}) == 3
    for p in planes:
        assert sorted(p[0, 0].tolist()) == [0, 85, 170, 255] and (p == p[0, 0]).all()
    y, x, c = np.meshgrid(np.arange(84), np.arange(84), np.arange(4), indexing="ij")
    assert np.array_equal(by["checker"], np.where((x + y + c) % 2, 255, 0))
    assert not by["all0"].any() and (by["all255"] == 255).all()
    assert np.array_equal(by["fixture2"], F.fixture_batch()[2])
    assert len([n for n in names if n.startswith("uniform")]) == 4
    assert np.array_equal(F.member_frames(45)[[0, 21, 22, 44]], fr[[0, 21, 0, 0]]) and F.frame_of(23) == names[1]


@pytest.mark.parametrize("kind", [KIND_ES, KIND_ES_VBN, KIND_GA, KIND_GA_LARGE], ids=["es", "vbn", "ga", "large"])
def test_members_are_what_the_cases_need(kind):
    import step_tap_support as S
    n = F.MAX_MEMBERS
    slot, off, scale = F.members(kind, F.NACT, n)
    hi = F.noise_of(kind).size - S.num_params(kind, F.NACT)
    assert off.min() == 0 == off[0] and off.max() == hi == off[3] and scale[0] != 0 and scale[3] != 0      # first and last legal slice, both read
    twins = np.arange(n) % 5 == 1
    assert (off[twins] == off[np.flatnonzero(twins) - 1]).all() and (scale[twins] == -scale[np.flatnonzero(twins) - 1]).all()
    assert len(set(off[~twins].tolist())) == (~twins).sum()          # otherwise every member has a noise offset of its own
    assert scale[:5].tolist() == [np.float32(v) for v in F.SCALES]
    assert set(slot.tolist()) == {KIND_GA: {1, 2, 3}, KIND_GA_LARGE: {1, 2}}.get(kind, {0})
    for m in (4, 32, 131):                                            # a prefix: member i is the same member at every count
        assert all(np.array_equal(a, b[:m]) for a, b in zip(F.members(kind, F.NACT, m), (slot, off, scale)))
    # above 32 members every frame sits at several positions; every frame meets every scale, and (GA kinds) more than one parent
    for f in range(22):
        at = np.flatnonzero(np.arange(131) % 22 == f)
        assert len(at) >= 5 and len(set(scale[at].tolist())) == 5 and len(set(slot[at].tolist())) == len(set(slot.tolist()))


def _oracle_engine(kind, nact, n):
    from oracle_engine import OracleEngine
    from vbn_support import OracleVBNEngine
    import oracle as O
    if kind == KIND_ES_VBN:
        e = OracleVBNEngine(n_actions=nact, max_members=n, ref_count=F.NREF)
    else:
        e = OracleEngine({KIND_ES: O.KIND_ES, KIND_GA: O.KIND_GA, KIND_GA_LARGE: O.KIND_GA_LARGE}[kind], n_actions=nact, max_members=n, ref_count=F.NREF)
    e.noise_upload(F.noise_of(kind))
    return e


@pytest.mark.parametrize("kind,nact,n", [(KIND_ES, 18, 27), (KIND_ES_VBN, 18, 23), (KIND_GA, 18, 27), (KIND_GA_LARGE, 18, 25), (KIND_ES, 3, 23)],
                         ids=["es", "vbn", "ga", "large", "es-3-actions"])
def test_harness_on_the_oracle_engine(kind, nact, n, oracle):
    """drive() on the oracle behind the engine surface, every frame at least once and the first ones twice: check() passes"""
    out = F.drive(_oracle_engine(kind, nact, n), kind, nact, n)
    F.check(out)
    assert len(out["y"][0]) == (4 if kind == KIND_GA_LARGE else 3) and ("bn" in out) == (kind in (KIND_ES, KIND_ES_VBN))
    # the members differ from each other: a harness that mixed two of them up could not pass
    lg = out["logits"]
    assert len({lg[i].tobytes() for i in range(n)}) == n
    if kind == KIND_ES:
        assert len({out["bn"][i].tobytes() for i in range(n)}) == n - len([i for i in range(n) if i % 5 == 2]) + 1   # (the scale-0 members are one vector)


def test_check_notices_what_it_must(oracle):
    """check() on a driven case with one thing moved: two members' frames swapped, one logit one ulp off, a wrong action, a frame byte lost"""
    kind, nact, n = KIND_GA, 18, 24
    out = F.drive(_oracle_engine(kind, nact, n), kind, nact, n)
    assert F.mismatches(out) == []

    def broken(**change):
        o = dict(out)
        o.update(change)
        return F.mismatches(o)

    lg = out["logits"].copy()
    lg[5, 7] = np.nextafter(lg[5, 7], np.float32(np.inf))
    bad = broken(logits=lg)
    assert len(bad) >= 1 and all(f == F.frame_of(5) for f, _ in bad) and "member 5 (%s) logits: 1 of 18 elements differ" % F.frame_of(5) in bad[0][1]
    assert "ga, 18 actions, 24 members" in bad[0][1]
    acts = out["actions"].copy()
    acts[3] = (acts[3] + 1) % nact
    assert {line.split(": ", 1)[1].split(":")[0] for _, line in broken(actions=acts)} == \
        {"member 3 (%s) action against the first maximum of its own logits" % F.frame_of(3), "member 3 (%s) action" % F.frame_of(3)}
    y = list(out["y"])
    y[1], y[23] = y[23], y[1]                                        # frames 1 and 1 (23 % 22), but two different members
    assert {int(line.split("member ")[1].split(" ")[0]) for _, line in broken(y=y)} == {1, 23}
    back = out["obs_back"].copy()
    back[11, 83, 83, 3] ^= 1
    (only,) = broken(obs_back=back)
    assert only[0] == F.frame_of(11) and "frame read back: 1 of 28224 elements differ" in only[1]
    # an engine that convolved member 2's frame for member 9: driven again with those two frames exchanged underneath
    e = _oracle_engine(kind, nact, n)
    real = e.env_set_observation
    e.env_set_observation = lambda obs: real(np.concatenate([obs[:2], obs[9:10], obs[3:9], obs[2:3], obs[10:]]))
    bad = F.mismatches(F.drive(e, kind, nact, n))
    assert {f for f, _ in bad} == {F.frame_of(2), F.frame_of(9)} and any("y1" in line for _, line in bad)
    with pytest.raises(AssertionError, match="mismatches, on frames"):
        F.check(dict(out, logits=lg))
