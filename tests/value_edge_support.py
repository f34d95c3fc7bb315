"""TEST-ONLY: parameter vectors at the ends of float32's range, for tests/test_value_edges_cpu.py and tests/test_gpu_value_edges.py.

Every other Atari forward test forms its weights as base + fl(sigma * noise) around a Xavier / normc start, so every weight, product,
partial sum and activation the matrix-core and packed-math kernels are compared on lies between about 1e-9 and 1e2.  Here ONE tensor
group of the base vector is multiplied by a power of two, so that the layer behind it lands on FLT_MIN (under classes) or on FLT_MAX (over
classes); everything else is the existing tap machinery (step_tap_support.oracle_taps, unchanged).

  groups()      G1 = conv1 w+b, G2 = conv2 w+b (LargeModel: G2 conv2, G2b conv3), G3 = fc w+b, G4 = out w+b of a kind's own flat layout;
                batch-norm beta / gamma are never touched; ModelVirtualBN is scaled in its native layout, before vbn_support.expand
  CLASSES       per kind: class -> (groups, e): the groups' entries times 2^e (np.ldexp through float64: exact wherever the result is
                normal), every other entry as it is.  U1..U4: e < 0, the scaled layer's output straddles FLT_MIN, and the evaluation's
                sigma is float32(0.02 * 2^e) (GA: the mutation power 0.005 * 2^e), so fl(sigma * eps) is itself subnormal in the scaled
                group and absorbed wherever the base is not zero.  O1..O4: e > 0, the scaled layer's output overflows in some elements
                and not in most; sigma stays 0.02.  BIG (GA): every group times 2^e, conv1 and conv2 finite, y3 partly infinite.
                The exponents are literals found on the CPU from the oracle alone; tests/test_value_edges_cpu.py holds each class to
                its mix condition.
  population    ES kinds: 5 antithetic pairs at noise offsets 0, 1, 2, 3 and N - P (every residue mod 4, the last legal slice, an odd
                count, a partial ring workgroup), seeds tap_seeds(10), taps at T = 1 and 3.  GA: ten single members of one parent over
                the same offsets, five with +power and five with -power (an evaluation takes the first seven).  A GA engine forms a
                root itself, so the scaled parent is handed over as ga_set_init_scale(normc factors, the groups times 2^e): the
                evaluation then runs both of the engine's own routes, children written out and on the fly.  LargeModel: the six
                genomes of step_tap_support.large_genomes(6) under model_scale_by with the groups times 2^e, the children's powers
                times 2^e in an under class.
  same_bits()   NaN where the oracle has NaN (any payload), equal bit patterns everywhere else: the sign of zero and of infinity count."""
import functools

import numpy as np

import oracle as O
import step_tap_support as S
from step_tap_support import KIND_ES, KIND_GA, KIND_GA_LARGE, KIND_ES_VBN, NACT

TAPS = (1, 3)                      # no episode can end by step 3: lengths == T is asserted by every evaluation
N_PAIRS = 5
SIGMA = 0.02
GA_SIGMA = S.GA_SIGMA
GA_PARENT = (100,)                 # the base of the GA classes: oracle.ga_rebuild([100]), formed as noise * normc factors (_normc_scale_by)
GA_EVAL_MEMBERS = 7
SEEDS = S.tap_seeds(2 * N_PAIRS)
FLT_MIN = np.float32(2.0 ** -126)

# class -> (groups, exponent).  Found with the oracle alone (member 0..9, T = 1) and held by tests/test_value_edges_cpu.py.
def _classes(u1, u2, u3, u4, o1, o2, o3, o4):
    return {"U1": (("G1",), u1), "U2": (("G2",), u2), "U3": (("G3",), u3), "U4": (("G4",), u4),
            "O1": (("G1",), o1), "O2": (("G2",), o2), "O3": (("G3",), o3), "O4": (("G4",), o4)}


CLASSES = {
    # Xavier start, virtual batch norm: O2 / O3 send NaN through the batch-norm statistics of the reference pass (wanted)
    KIND_ES: _classes(-124, -125, -126, -125, 128, 128, 127, 128),
    KIND_ES_VBN: _classes(-125, -125, -126, -125, 128, 127, 127, 128),
    # normc start, no batch norm: O1's y2 holds +-inf and NaN, its y3 is all NaN and its logits are the out bias (relu of NaN is +0);
    # O3's logits are all NaN; out weights of 0.1 / sqrt(256) need 2^133 for an infinite logit and are no longer finite at 2^134
    KIND_GA: dict(_classes(-124, -124, -124, -120, 127, 128, 129, 133), BIG=(("G1", "G2", "G3", "G4"), 43)),
    # LargeModel (scale_by times 2^e: the engine forms a root as noise * scale_by); the fc's output is y4
    KIND_GA_LARGE: {"U1": (("G1",), -124), "U3": (("G3",), -123), "O1": (("G1",), 128), "O3": (("G3",), 130)},
}
# the layer whose output a class's mix condition is about: index into (y1, y2, y3, logits) / LargeModel (y1, y2, y3, y4, logits)
SCALED_OUTPUT = {"U1": 0, "O1": 0, "U2": 1, "O2": 1, "U3": 2, "O3": 2, "U4": 3, "O4": 3, "BIG": 2}
LARGE_SCALED_OUTPUT = {"U1": 0, "O1": 0, "U3": 3, "O3": 3}


def is_under(cls):
    return cls.startswith("U")


def _layout(kind, nact=NACT):
    return O.layout({KIND_GA: O.KIND_GA, KIND_GA_LARGE: O.KIND_GA_LARGE}.get(kind, O.KIND_ES), nact)


@functools.lru_cache(maxsize=None)
def _groups(kind, nact):
    if kind == KIND_ES_VBN:
        from dne_hip import _lib, policies
        spec, _ = policies.flat_layout(_lib.KIND_ES_VBN, nact)
        rng = lambda name: (spec[name][0], int(np.prod(spec[name][1])))
        return {"G1": (rng("layer1/conv1/w"),), "G2": (rng("layer2/conv2/w"),), "G3": (rng("layer3/fc/w"),),
                "G4": (rng("layer4/out/w"), rng("layer4/out/b"))}
    L = _layout(kind, nact)
    if kind == KIND_GA_LARGE:
        return {"G1": ((L.c1w, 8192), (L.c1b, 32)), "G2": ((L.c2w, 32768), (L.c2b, 64)), "G2b": ((L.c3w, 36864), (L.c3b, 64)),
                "G3": ((L.fcw, 7744 * 512), (L.fcb, 512)), "G4": ((L.ow, 512 * nact), (L.ob, nact))}
    return {"G1": ((L.c1w, 4096), (L.c1b, 16)), "G2": ((L.c2w, 8192), (L.c2b, 32)), "G3": ((L.fcw, 3872 * 256), (L.fcb, 256)),
            "G4": ((L.ow, 256 * nact), (L.ob, nact))}


def groups(kind, nact=NACT):
    """{group: ((offset, count), ...)} in the kind's own flat layout"""
    return _groups(int(kind), int(nact))


def scale_groups(vec, kind, cls, nact=NACT):
    """vec with the class's groups times 2^e, every other entry as it is"""
    names, e = CLASSES[kind][cls]
    out = np.array(vec, np.float32)
    for g in names:
        for off, n in groups(kind, nact)[g]:
            out[off:off + n] = np.ldexp(out[off:off + n].astype(np.float64), e).astype(np.float32)
    assert np.isfinite(out).all(), (kind, cls)       # the contract's domain: every FINITE parameter vector
    return out


def sigma_of(kind, cls):
    """the evaluation's sigma (GA: the mutation power) of a class, as the float32 the engine takes"""
    s = GA_SIGMA if kind == KIND_GA else SIGMA
    return float(np.float32(np.ldexp(s, CLASSES[kind][cls][1]))) if is_under(cls) else s


def pair_indices(kind, nact=NACT):
    return np.array([0, 1, 2, 3, S.NOISE_LEN - S.num_params(kind, nact)], np.int64)


# ---- ES / ModelVirtualBN -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _normc_scale_by():
    """normc_tensor of oracle/dne_oracle.c as a per-parameter factor: every weight of a column times std / sqrt(sum of squares, added row by
    row in float32), every bias times 0 -- so that noise[s0 : s0 + P] * scale_by is oracle.ga_rebuild([s0]) (a zeroed bias as +-0), and a
    GA engine forms the class's parent itself from ga_set_init_scale(scale_by times 2^e) (tests/test_value_edges_cpu.py holds both)"""
    L, x = _layout(KIND_GA), S.small_noise()[GA_PARENT[0]:GA_PARENT[0] + S.P_GA]
    sb = np.zeros(S.P_GA, np.float32)
    for off, K, C, std in ((L.c1w, 256, 16, 1.0), (L.c2w, 256, 32, 1.0), (L.fcw, 3872, 256, 1.0), (L.ow, 256, NACT, 0.1)):
        w = x[off:off + K * C].reshape(K, C)
        ss = np.zeros(C, np.float32)
        for k in range(K):
            ss = ss + w[k] * w[k]
        sb[off:off + K * C] = np.broadcast_to(np.float32(std) / np.sqrt(ss), (K, C)).reshape(-1)
    assert sb.dtype == np.float32
    sb.setflags(write=False)
    return sb


@functools.lru_cache(maxsize=None)
def ga_scale_by(cls):
    """what ga_set_init_scale gets for a GA class: the normc factors, the class's groups times 2^e"""
    sb = scale_groups(_normc_scale_by(), KIND_GA, cls)
    sb.setflags(write=False)
    return sb


@functools.lru_cache(maxsize=None)
def _base(kind, cls):
    if kind == KIND_GA:              # = scale_groups(oracle.ga_rebuild(GA_PARENT)) up to the sign of a zero bias
        with np.errstate(all="ignore"):
            b = O.ga_gpu_rebuild(S.small_noise(), GA_PARENT, ga_scale_by(cls))
        assert np.isfinite(b).all(), cls
    else:
        b = scale_groups(S.base_theta(kind), kind, cls)
    b.setflags(write=False)
    return b


def base(kind, cls):
    """the class's base vector in the kind's native layout (ES kinds: what set_theta gets; GA: the parent's slot)"""
    return _base(int(kind), cls)


def es_member(kind, cls, m):
    """(noise offset, signed sigma) of member m of the 5 pairs"""
    s = np.float32(sigma_of(kind, cls))
    return int(pair_indices(kind)[m // 2]), float(s if m % 2 == 0 else -s)


def ga_members(cls, n=2 * N_PAIRS):
    """(offset int64 [n], power float32 [n]) of the GA members: the five offsets with +power, then the same with -power"""
    off = np.concatenate([pair_indices(KIND_GA), pair_indices(KIND_GA)])[:n]
    s = np.float32(sigma_of(KIND_GA, cls))
    return off.astype(np.int64), np.where(np.arange(n) < N_PAIRS, s, -s).astype(np.float32)


def ga_genomes(cls, n=GA_EVAL_MEMBERS):
    """the first n GA members as genomes with powers, (root, (offset, power)): what ga_eval_powers takes behind ga_set_init_scale(ga_scale_by(cls))"""
    off, power = ga_members(cls, n)
    return [(GA_PARENT[0], (int(o), float(p))) for o, p in zip(off, power)]


def member(kind, cls, m):
    """(noise offset, signed scale) of member m of a kind's population"""
    if kind != KIND_GA:
        return es_member(kind, cls, m)
    off, power = ga_members(cls)
    return int(off[m]), float(power[m])


def member_theta(kind, cls, m):
    """member m's vector as the oracle runs it: base + fl(scale * noise[off : off + P]), two float32 roundings (ModelVirtualBN: expanded)"""
    off, sc = member(kind, cls, m)
    b = base(kind, cls)
    with np.errstate(all="ignore"):
        th = (b + (np.float32(sc) * S.small_noise()[off:off + b.size]).astype(np.float32)).astype(np.float32)
    if kind == KIND_ES_VBN:
        from vbn_support import expand
        th = expand(th, NACT)
    return th


@functools.lru_cache(maxsize=None)
def _taps(kind, cls, m):
    ref = S.ref_batch() if kind != KIND_GA else None
    return S.oracle_taps(_layout(kind), member_theta(kind, cls, m), ref, int(SEEDS[m]), TAPS)


def taps(kind, cls, m):
    """{T: tap} for T in TAPS of member m of a class (kinds ES, ES_VBN, GA), cached: every regime shares it"""
    return _taps(int(kind), cls, int(m))


@functools.lru_cache(maxsize=None)
def _moments(kind, cls, m):
    bn, mom = O.es_ref_pass_moments(_layout(kind), member_theta(kind, cls, m), S.ref_batch())
    assert bits_differ(bn, _taps(kind, cls, m)[1]["bn"]) is None
    return mom


def moments(kind, cls, m):
    """the batch means / variances of member m's reference pass (get_bn_moments' 608 floats).  Under U1 conv1's means are subnormal and its
    variances underflow: ModelVirtualBN's batch-norm shift absorbs a flushed y1 everywhere behind bn1, so there the moments are what shows
    a conv1 that flushes (a library built to flush denormals passes every other comparison of that kind's U1 cases)"""
    return _moments(int(kind), cls, int(m))


# ---- LargeModel ---------------------------------------------------------------------------------------------------------------------------
N_LARGE = 6


@functools.lru_cache(maxsize=None)
def large_scale_by(cls):
    """ga_gpu.model_scale_by with the class's groups times 2^e: the engine forms a root as noise * scale_by, so this IS the scaled base"""
    from dne_hip import ga_gpu
    sb = scale_groups(ga_gpu.model_scale_by(NACT, KIND_GA_LARGE), KIND_GA_LARGE, cls)
    sb.setflags(write=False)
    return sb


def large_genomes(cls):
    """step_tap_support.large_genomes(6); in an under class the two children's powers times 2^e (float32)"""
    e = CLASSES[KIND_GA_LARGE][cls][1] if is_under(cls) else 0
    return [tuple((c[0], float(np.float32(np.ldexp(c[1], e)))) if isinstance(c, tuple) else c for c in g) for g in S.large_genomes(N_LARGE)]


@functools.lru_cache(maxsize=None)
def large_taps(cls, m):
    with np.errstate(all="ignore"):
        th = O.ga_gpu_rebuild(S.big_noise(), large_genomes(cls)[m], large_scale_by(cls))
    return S.oracle_taps(_layout(KIND_GA_LARGE), th, None, int(S.tap_seeds(N_LARGE)[m]), TAPS, large=True)


# ---- dne_act: members 0..9 of a class on frames_support's frames ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _act_expected(kind, cls, m):
    import frames_support as F
    th, frame = member_theta(kind, cls, m), F.frames()[m % len(F.frames())]
    L = _layout(kind)
    bn, mom = O.es_ref_pass_moments(L, th, F.ref_batch()) if kind != KIND_GA else (None, None)
    *y, lg = O.forward_debug(L, th, bn, frame)
    return dict(bn=bn, mom=mom, y=tuple(y), logits=lg, action=O.act(L, th, bn, frame)[0])


def act_expected(kind, cls, m):
    """the oracle's bn and batch moments, (y1, y2, y3), logits and action of member m on frame m of frames_support (its 8 reference frames), cached"""
    return _act_expected(int(kind), cls, int(m))


# ---- the comparison rule ------------------------------------------------------------------------------------------------------------------
def bits_differ(got, want):
    """None if got holds NaN (any payload) wherever want does and want's bit patterns everywhere else, otherwise a report"""
    g, w = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    if g.shape != w.shape:
        return "shape %s, not %s" % (g.shape, w.shape)
    nan = np.isnan(w)
    if np.isnan(g[nan]).all() and np.array_equal(g[~nan].view(np.int32), w[~nan].view(np.int32)):
        return None
    from test_gpu_step_taps import _ulp_report
    shown = np.where(nan & np.isnan(g), w, g)        # (a NaN of another payload is no difference)
    return "%s; NaN wanted at %d places, %d of them NaN" % (_ulp_report(shown, w), int(nan.sum()), int(np.isnan(g[nan]).sum()))


def same_bits(got, want, *ctx):
    bad = bits_differ(got, want)
    assert bad is None, (ctx, bad)


def census(x):
    """(non-zero subnormal, normal, +-inf, NaN, zero) counts of an array"""
    x = np.asarray(x, np.float32)
    a = np.abs(x)
    with np.errstate(invalid="ignore"):
        return dict(subnormal=int(((a > 0) & (a < FLT_MIN)).sum()), normal=int((np.isfinite(x) & (a >= FLT_MIN)).sum()),
                    inf=int(np.isinf(x).sum()), nan=int(np.isnan(x).sum()), zero=int((a == 0).sum()), size=int(x.size))
