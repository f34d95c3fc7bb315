"""TEST-ONLY: frames the SynthAtari fixture never draws, and the one case every dne_act route is held to on them.

Inside an evaluation the convolutions only ever see rendered frames: 208 of the 256 byte values, four stacked channels that mostly agree, one
value filling a fifth of all bytes (testing).  Arbitrary frames reach the device through env_set_observation + act, and which
kernels an act launches follows from the member count alone (csrc/plan.h: act_window, dne_debug_plan_act).  Here:

  frames()        22 crafted frames [84][84][4]: every byte value in every channel, only values the fixture lacks, channels that disagree
                  everywhere, single bytes in the corners and off the tile grid, constant planes, the extremes, one fixture frame as control
  members()       member i of a kind: its base slot, noise offset and scale -- the same for every member count, so the oracle side of member
                  i is worked out once per session (expected()) whatever cases use it; member i looks at frame i % 22
  ACT_ROWS ...    the kernels an act of n members launches by default, as literals: a default that moves must fail a test
  drive()         the calls of a case on an engine -- the HIP engine or tests/oracle_engine.py, the same code for both
  check()         every member of a driven case against expected(), np.array_equal, no tolerance

tests/test_frames_cpu.py holds the frame set to what it is for and runs drive() + check() on the oracle behind the engine surface;
tests/test_gpu_frames.py runs them on the GPU at every width where the act plan changes."""
import functools

import numpy as np

import oracle as O
import step_tap_support as S
from step_tap_support import KIND_ES, KIND_ES_VBN, KIND_GA, KIND_GA_LARGE

NACT = 18
NREF = 8                                            # reference frames of the ES kinds' virtual batch norm
MAX_MEMBERS = 257                                   # the widest case
SCALES = (0.02, -0.02, 0.0, 0.5, -0.1)              # member i: SCALES[i % 5]; the -0.02 member is the antithetic twin of the member before it
GA_SIGMA = 0.005
GA_PARENTS = ([100], [200_000, 7], [2_900_000, 5, 123_456])         # base slots 1..3 (tests/test_gpu_parity.py::test_forward_ga_bit_exact)
LARGE_PARENTS = ((1234,), (3_000_000, (77, 0.004)))                 # base slots 1..2, seeds with powers (tests/test_gpu_large.py)
KIND_NAMES = {KIND_ES: "es", KIND_ES_VBN: "vbn", KIND_GA: "ga", KIND_GA_LARGE: "large"}
IMPULSES = ((0, 0, 0), (0, 83, 1), (83, 0, 2), (83, 83, 3), (3, 4, 0), (4, 3, 3), (41, 42, 1), (80, 79, 2))     # (y, x, c)
PLANES = ((0, 85, 170, 255), (255, 170, 85, 0), (85, 255, 0, 170))

# dne_act's kernels by member count with no knob set: (members, conv path, (s1, s2) of k_conv1 / k_conv2 or None, fc kernel).  Literals on
# purpose: tests/test_plan_cpu.py derives the same counts from the knobs, the GPU cases assert these rows before they launch anything.
ACT_ROWS = ((32, "k_conv12t", None, "k_fc_tail"), (33, "k_conv12t", None, "k_fc_cols"), (64, "k_conv12t", None, "k_fc_cols"),
            (65, "split", (4, 2), "k_fc_cols"), (96, "split", (4, 2), "k_fc_cols"), (97, "split", (4, 2), "k_fc"),
            (128, "split", (4, 2), "k_fc"), (129, "k_conv12", None, "k_fc"), (131, "k_conv12", None, "k_fc"))
ACT_KNOB_ROWS = (({"DNE_CONV12T_MAX": "0"}, 32, "split", (7, 4), "k_fc_tail"),      # conv1_body over 7 workgroups, conv2 over 4
                 ({"DNE_CONV_FUSED": "0"}, 257, "split", (1, 2), "k_fc"))           # k_conv1 with one workgroup per member
ACT_LARGE_ROWS = ((96, 4, "k_lfc_cols"), (97, 4, "k_lfc"), (129, 2, "k_lfc"), (257, 1, "k_lfc"))   # (members, workgroups per member of the convolutions, fc)


# ---- the frames ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_batch():
    """the 128 frames of the reference batch: what the fixture's renderer draws"""
    return O.get_ref_batch(seed=0, batch_size=128, nact=NACT)


@functools.lru_cache(maxsize=None)
def _absent_values():
    return tuple(int(v) for v in np.setdiff1d(np.arange(256), np.unique(fixture_batch())))


def absent_values():
    """the byte values no pixel of fixture_batch() has, computed"""
    return np.array(_absent_values(), np.uint8)


@functools.lru_cache(maxsize=None)
def _frames():
    y, x, c = np.meshgrid(np.arange(84), np.arange(84), np.arange(4), indexing="ij")
    out = [("ramp", (13 * y + 7 * x + 61 * c) % 256)]
    for k in range(2):
        out.append(("absent%d" % k, np.random.RandomState(500 + k).choice(absent_values(), size=(84, 84, 4))))
    for k in range(4):
        out.append(("uniform%d" % k, np.random.RandomState(600 + k).randint(0, 256, (84, 84, 4))))
    for p in PLANES:
        out.append(("planes-%d-%d-%d-%d" % p, np.broadcast_to(np.array(p), (84, 84, 4))))
    for at in IMPULSES:
        f = np.zeros((84, 84, 4), np.int64)
        f[at] = 255
        out.append(("impulse-y%d-x%d-c%d" % at, f))
    out.append(("checker", np.where((x + y + c) % 2 == 1, 255, 0)))
    out.append(("all0", np.zeros((84, 84, 4), np.int64)))
    out.append(("all255", np.full((84, 84, 4), 255)))
    out.append(("fixture2", fixture_batch()[2]))
    names = tuple(n for n, _ in out)
    arr = np.stack([np.asarray(f).astype(np.uint8) for _, f in out])
    arr.setflags(write=False)
    return names, arr


def frame_names():
    return _frames()[0]


def frames():
    """[22][84][84][4] uint8, read-only"""
    return _frames()[1]


def frame_of(i):
    """the name of the frame member i looks at"""
    return frame_names()[i % len(frame_names())]


def member_frames(n):
    return np.ascontiguousarray(frames()[np.arange(n) % len(frames())])


# ---- the members --------------------------------------------------------------------------------------------------------------------------
def noise_of(kind):
    return S.big_noise() if kind == KIND_GA_LARGE else S.small_noise()


@functools.lru_cache(maxsize=None)
def _ref(nact):
    return O.get_ref_batch(seed=0, batch_size=NREF, nact=nact)


def ref_batch(nact=NACT):
    return _ref(int(nact))


@functools.lru_cache(maxsize=None)
def _members(kind, nact):
    hi = noise_of(kind).size - S.num_params(kind, nact)                  # the last legal offset
    i = np.arange(MAX_MEMBERS)
    off = np.random.RandomState(20261).randint(0, hi + 1, MAX_MEMBERS).astype(np.int64)
    off[0], off[3] = 0, hi                                               # (scales 0.02 and 0.5: both slices are really read)
    twin = i % 5 == 1
    off[twin] = off[i[twin] - 1]                                         # (offset, +0.02), (the same offset, -0.02)
    scale = np.array(SCALES, np.float32)[i % 5]
    if kind == KIND_GA:
        slot = 1 + i % 3
    elif kind == KIND_GA_LARGE:
        slot = 1 + (i + i // len(frame_names())) % 2                     # (22 frames: plain i % 2 would tie a frame to one parent)
    else:
        slot = np.zeros(MAX_MEMBERS, np.int64)
    return slot.astype(np.int32), off, scale


def members(kind, nact, n):
    """(slot, offset, scale) of members 0 .. n-1: a prefix of one list per kind, so member i is the same member in every case"""
    assert 4 <= n <= MAX_MEMBERS
    slot, off, scale = _members(int(kind), int(nact))
    return slot[:n].copy(), off[:n].copy(), scale[:n].copy()


@functools.lru_cache(maxsize=None)
def _base_vectors(kind, nact):
    if kind in (KIND_ES, KIND_ES_VBN):
        return {0: S.base_theta(kind, nact)}
    if kind == KIND_GA:
        L = O.layout(O.KIND_GA, nact)
        return {s: O.ga_rebuild(L, S.small_noise(), chain, GA_SIGMA) for s, chain in enumerate(GA_PARENTS, 1)}
    from dne_hip import ga_gpu
    sb = ga_gpu.model_scale_by(nact, KIND_GA_LARGE)
    return {s: O.ga_gpu_rebuild(S.big_noise(), g, sb) for s, g in enumerate(LARGE_PARENTS, 1)}


def base_vectors(kind, nact=NACT):
    """{base slot: vector} of a kind, from the oracle (native layout)"""
    return _base_vectors(int(kind), int(nact))


def _layout(kind, nact):
    return O.layout({KIND_GA: O.KIND_GA, KIND_GA_LARGE: O.KIND_GA_LARGE}.get(kind, O.KIND_ES), nact)


@functools.lru_cache(maxsize=None)
def _expected(kind, nact, i):
    slot, off, scale = (a[i] for a in _members(kind, nact))
    base = base_vectors(kind, nact)[int(slot)]
    # base + fl(scale * noise[off : off + P]): two float32 roundings, as every kernel forms a member's weight
    th = (base + (np.float32(scale) * noise_of(kind)[off:off + base.size]).astype(np.float32)).astype(np.float32)
    if kind == KIND_ES_VBN:
        from vbn_support import expand
        th = expand(th, nact)
    L, frame = _layout(kind, nact), frames()[i % len(frames())]
    if kind == KIND_GA_LARGE:
        *y, lg = O.forward_large_debug(L, th, frame)
        bn = mom = None
    else:
        bn, mom = O.es_ref_pass_moments(L, th, ref_batch(nact)) if kind != KIND_GA else (None, None)
        *y, lg = O.forward_debug(L, th, bn, frame)
    return dict(bn=bn, mom=mom, y=tuple(y), logits=lg, action=O.act(L, th, bn, frame)[0])


def expected(kind, nact, i):
    """the oracle's values of member i on its frame: bn / mom (ES kinds), y = (y1, y2, y3[, y4]), logits, action -- cached per session"""
    return _expected(int(kind), int(nact), int(i))


# ---- a case on an engine -------------------------------------------------------------------------------------------------------------------
def act_facts():
    """the planner's facts under dne_act: dne_set_members leaves the members as (slot, offset, scale) triples, nothing written out -- and with
    single members under the empty plan no other fact is read"""
    return dict(members_materialized=0)


def drive(e, kind, nact, n):
    """The calls of one case on an engine that has its noise table: bases, members, frames, reference pass (ES kinds), act -- then everything
    check() compares, read back.  The same code drives the HIP engine and the oracle behind the engine surface."""
    es = kind in (KIND_ES, KIND_ES_VBN)
    want = base_vectors(kind, nact)
    if es:
        e.set_theta(want[0])
        e.set_ref_batch(ref_batch(nact))
    elif kind == KIND_GA:
        for s, chain in enumerate(GA_PARENTS, 1):
            assert np.array_equal(e.ga_rebuild(s, chain, GA_SIGMA), want[s]), ("ga_rebuild", chain)
    else:
        from dne_hip import ga_gpu
        e.ga_set_init_scale(ga_gpu.model_scale_by(nact, KIND_GA_LARGE))
        for s, g in enumerate(LARGE_PARENTS, 1):
            assert np.array_equal(e.ga_rebuild_powers(s, g), want[s]), ("ga_rebuild_powers", g)
    e.set_members(*members(kind, nact, n))
    obs = member_frames(n)
    e.env_set_observation(obs)
    out = dict(kind=kind, nact=nact, n=n, obs=obs)
    if es:
        e.ref_pass(n)
        out["bn"], out["mom"] = e.get_bn(n), e.get_bn_moments(n)
    out["actions"], out["logits"] = e.act(n)
    out["y"] = [e.debug_activations_large(i) if kind == KIND_GA_LARGE else e.debug_activations(i) for i in range(n)]
    out["obs_back"] = e.env_observation(n)
    out["redzones"] = e.check_redzones()
    return out


def _differing(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return "shape %s, not %s" % (got.shape, want.shape) if got.shape != want.shape else "%d of %d elements differ" % (int((got != want).sum()), want.size)


def mismatches(out):
    """every (member, quantity) of a driven case that is not np.array_equal to the oracle's: (frame name, one line naming the kind, the member
    count, the member, its frame and how many elements differ)"""
    kind, nact, n = out["kind"], out["nact"], out["n"]
    bad = []

    def hold(i, what, got, want):
        if not np.array_equal(got, want):
            bad.append((frame_of(i), "%s, %d actions, %d members: member %d (%s) %s: %s" % (KIND_NAMES[kind], nact, n, i, frame_of(i), what, _differing(got, want))))

    assert out["logits"].shape == (n, nact) and out["actions"].shape == (n,)
    for i in range(n):
        want = expected(kind, nact, i)
        if want["bn"] is not None:
            hold(i, "bn", out["bn"][i], want["bn"])
            hold(i, "bn moments", out["mom"][i], want["mom"])
        assert len(out["y"][i]) == len(want["y"])
        for k, (got, w) in enumerate(zip(out["y"][i], want["y"]), 1):
            hold(i, "y%d" % k, got, w)
        hold(i, "logits", out["logits"][i], want["logits"])
        hold(i, "action against the first maximum of its own logits", int(out["actions"][i]), S.argmax_first(out["logits"][i]))
        hold(i, "action", int(out["actions"][i]), int(want["action"]))
        hold(i, "frame read back", out["obs_back"][i], out["obs"][i])
    return bad


def check(out):
    bad = mismatches(out)
    assert not bad, "%d mismatches, on frames %s:\n%s" % (len(bad), sorted({f for f, _ in bad}), "\n".join(line for _, line in bad[:40]))
    assert out["redzones"] == 0
