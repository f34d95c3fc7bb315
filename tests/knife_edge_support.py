"""TEST-ONLY: knife-edge members -- populations whose step-T decision flips between two noise tables that differ in ONE float32 per member,
by one unit in the last place.

Inside an evaluation the policy head (bn3 + relu, the 256 x A / 512 x A output layer, + bias, first-maximum argmax, commit) is seen only
through the action it commits (RAM byte 38 of the recorded trajectory).  A member's output bias is fl(base + fl(scale * noise[e])) and its
logit fl(t_b + bias_b): monotone in the one table entry e = window + (offset of out/b) + b, and nothing else of the network reads that entry.
So the test, which owns the table, bisects e over the integer ordering of float32 until two ADJACENT floats x_lo < x_hi are left between which
the oracle's decision at step T flips from the top action a to column b.  On one of the two tables logit_a and logit_b are bit-equal (the
first maximum decides: b wins the tie iff b < a), on the other they are adjacent floats.  A head that is one ulp off on either logit, or
breaks the tie the other way, commits another action than the oracle on at least one of the two tables.

Oracle only, no GPU; everything is cached per session (functools.lru_cache), like step_tap_support.es_member_taps.  The tables are
generated (seeded randn), one window of P floats per pair / per GA or LargeModel seed, pairwise disjoint: an edited entry is no other
member's parameter (its antithetic twin reads it with the opposite sign: each member of a pair takes a column that is never the twin's top
or chosen column up to step T, so the twin only sees a losing logit move DOWN).

The bisection itself is arithmetic: one forward pass of the oracle at step T's observation gives y3 (LargeModel y4) and the logits, the
pre-bias sum t_b comes from head_sums() below (out_raw_k of oracle/dne_oracle.c in numpy, asserted bit-equal to the oracle's logits on
every member), and a probe of x costs three float32 operations.  What COUNTS as a knife-edge is then recomputed from the two final tables
alone by full T-step oracle rollouts (verify in _build_case)."""
import functools

import numpy as np

import oracle as O
import step_tap_support as S
from step_tap_support import KIND_ES, KIND_GA, KIND_GA_LARGE, KIND_ES_VBN, NACT

SIGMA = 0.02
F32 = np.float32


# ---- float32 as ordered integers ---------------------------------------------------------------------------------------------------------
def key(x):
    """position of a float32 in the total order of finite floats (+0 and -0 both 0): adjacent floats have adjacent keys"""
    i = int(np.asarray(x, F32).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def unkey(k):
    bits = k if k >= 0 else (0x80000000 | -k)
    return np.array(bits, np.uint32).view(F32)[()]


def ulps(x, y):
    return abs(key(x) - key(y))


# ---- the head in numpy: out_raw_k of oracle/dne_oracle.c, and deliberately wrong versions of it ---------------------------------------------
def activate(y, bn):
    """bn3 + relu of the oracle (bn_relu: multiply, add, compare; GA kinds: relu): y3 [256] -> a3, LargeModel y4 [512] -> a4"""
    t = np.asarray(y, F32)
    if bn is not None:
        t = (t * bn[96:352]).astype(F32)
        t = (t + bn[352:608]).astype(F32)
    return np.where(t > 0, t, F32(0.0)).astype(F32)


def group_sums(w, a):
    """S[g][col]: the products a[k] * w[k][col] (one rounding each) of every 64 consecutive k, summed by tree64 (neighbours first)"""
    t = (a[:, None] * w).astype(F32).reshape(-1, 64, w.shape[1])
    while t.shape[1] > 1:
        t = (t[:, 0::2] + t[:, 1::2]).astype(F32)
    return t[:, 0]


def _fold(S_):
    t = ((S_[0] + S_[1]).astype(F32) + (S_[2] + S_[3]).astype(F32)).astype(F32)
    if len(S_) == 8:
        t = (t + ((S_[4] + S_[5]).astype(F32) + (S_[6] + S_[7]).astype(F32)).astype(F32)).astype(F32)
    return t


def head_sums(w, a):
    """the logits before the bias: ((S0+S1)+(S2+S3)) [+ ((S4+S5)+(S6+S7))]"""
    return _fold(group_sums(w, a))


def head_logits(w, bias, a):
    return (head_sums(w, a) + bias).astype(F32)


def argmax_ge(x):
    best = 0
    for i in range(1, len(x)):
        if x[i] >= x[best]:
            best = i
    return best


# a head: (w [K][A], bias [A], a [K], twin_bias [A] or None) -> action
def head_oracle(w, bias, a, twin_bias):
    return S.argmax_first(head_logits(w, bias, a))


def head_ge(w, bias, a, twin_bias):
    """`>=` in the argmax loop: the LAST maximum"""
    return argmax_ge(head_logits(w, bias, a))


def head_ulp(col, up):
    """one logit moved by one unit in the last place"""
    def head(w, bias, a, twin_bias):
        lg = head_logits(w, bias, a)
        lg[col] = np.nextafter(lg[col], F32(np.inf if up else -np.inf))
        return S.argmax_first(lg)
    return head


def head_serial(w, bias, a, twin_bias):
    """the products summed as one serial chain over k instead of tree64 per group"""
    p = (a[:, None] * w).astype(F32)
    return S.argmax_first((np.add.accumulate(p, axis=0, dtype=F32)[-1] + bias).astype(F32))


def head_bias_first(w, bias, a, twin_bias):
    """the bias added to the first group sum instead of last"""
    S_ = group_sums(w, a).copy()
    S_[0] = (S_[0] + bias).astype(F32)
    return S.argmax_first(_fold(S_))


def head_twin_bias(w, bias, a, twin_bias):
    """the bias of the pair's other member"""
    return S.argmax_first(head_logits(w, bias if twin_bias is None else twin_bias, a))


# ---- populations -------------------------------------------------------------------------------------------------------------------------
class Population:
    """n members on one dedicated table.  theta(table, m): the member's vector as the oracle runs it, built from `table` the way the engine
    kind builds it.  entry0[m]: table position of the member's output-bias column 0 (-1: the member has no table entry behind its bias with
    a nonzero scale -- it stays in the population, compared but never an edge); scale[m] / bias0[m]: bias_b = fl(bias0[b] + fl(scale * x))"""

    def __init__(self, name, kind, nact, taps, table, seeds, scale, entry0, bias0, twin, theta, ref, **extra):
        self.name, self.kind, self.nact, self.taps, self.table, self.seeds = name, kind, nact, tuple(taps), table, seeds
        self.scale, self.entry0, self.bias0, self.twin, self.theta, self.ref = np.asarray(scale, F32), entry0, bias0, twin, theta, ref
        self.n = len(seeds)
        self.large = kind == KIND_GA_LARGE
        self.L = O.layout({KIND_ES: O.KIND_ES, KIND_ES_VBN: O.KIND_ES, KIND_GA: O.KIND_GA, KIND_GA_LARGE: O.KIND_GA_LARGE}[kind], nact)
        self.per_step_ram = kind in (KIND_ES, KIND_ES_VBN)          # the ES engines record every step's RAM, the GA engines the final one
        self.__dict__.update(extra)
        table.setflags(write=False)

    def rollout(self, table, m, taps):
        return S.oracle_taps(self.L, self.theta(table, m), self.ref, int(self.seeds[m]), tuple(taps), self.large)

    def head_inputs(self, table, m, tap):
        """(w, bias, a, twin_bias) of the member's last decision in `tap`"""
        L, th = self.L, self.theta(table, m)
        K = 512 if self.large else 256
        tw = self.twin[m]
        twin_bias = None if tw is None else self.theta(table, tw)[L.ob:L.ob + L.nact].copy()
        return (th[L.ow:L.ow + K * L.nact].reshape(K, L.nact).copy(), th[L.ob:L.ob + L.nact].copy(), activate(tap["y"][-1], tap["bn"]), twin_bias)


def _randn(seed, n):
    return np.random.RandomState(seed).randn(n).astype(F32)


def es_windows(P):
    """11 pairwise disjoint windows of P floats and the table length: the alignment classes of step_tap_support.edge_indices -- the first
    legal slice, a window that abuts it, start residues 1, 2, 3 (mod 4), a 16-byte aligned start that is not 256-byte aligned, a 256-byte
    aligned start (64 floats), an odd start one short of 512 bytes, a window one float behind its neighbour, one that abuts that, and the
    last legal slice -- in an order that is not the table's"""
    def up(x, mod, res):
        return x + (res - x) % mod
    s = [0, P]
    for mod, res in ((4, 1), (4, 2), (4, 3), (64, 4), (64, 0), (128, 127)):
        s.append(up(s[-1] + P, mod, res))
    s.append(s[-1] + P + 1)
    s.append(s[-1] + P)
    s.append(s[-1] + P + 5)
    N = s[-1] + P
    s = np.array(s, np.int64)
    assert all(b - a >= P for a, b in zip(s[:-1], s[1:])) and s[1] == P and s[9] - s[8] == P and s[8] - s[7] == P + 1
    assert [int(x) % 4 for x in s[2:5]] == [1, 2, 3] and s[5] % 64 == 4 and s[6] % 64 == 0 and s[7] % 128 == 127
    return s[[6, 0, 10, 3, 8, 1, 5, 9, 2, 7, 4]], int(N)


# the seeds of the generated tables, chosen so that the oracle alone meets the conditions of tests/test_knife_edge_cpu.py
TABLE_SEED = {(KIND_ES, 18): 2024, (KIND_ES_VBN, 18): 2025, (KIND_ES, 3): 2054, (KIND_ES, 17): 2027, (KIND_GA, 18): 2031, (KIND_GA_LARGE, 18): 2029}


def _bias_offset(kind, nact):
    """offset of the output biases in the kind's OWN flat layout (where the engine's member reads them in its window)"""
    from dne_hip import policies
    spec, _ = policies.flat_layout(kind, nact)
    name = [k for k in spec if k.endswith("out/b") or k.endswith("out/biases")]
    assert len(name) == 1 and int(np.prod(spec[name[0]][1])) == nact, (kind, spec)
    return spec[name[0]][0]


@functools.lru_cache(maxsize=None)
def es_population(kind, nact=NACT):
    """the 11 antithetic pairs of the tap tests (sigma 0.02, episodes tap_seeds(22)) on windows of their own"""
    P = S.num_params(kind, nact)
    idx, N = es_windows(P)
    table = _randn(TABLE_SEED[kind, nact], N)
    n = 2 * len(idx)
    ob = _bias_offset(kind, nact)
    base = S.base_theta(kind, nact)
    scale = np.array([F32(SIGMA) if m % 2 == 0 else -F32(SIGMA) for m in range(n)], F32)

    def theta(tab, m):
        return S.es_member_theta(kind, int(idx[m // 2]), float(scale[m]), nact, noise=tab)

    return Population("es" if kind == KIND_ES else "vbn", kind, nact, S.TAP_STEPS if nact == NACT else S.TAP_STEPS[:1], table, S.tap_seeds(n), scale,
                      entry0=[int(idx[m // 2]) + ob for m in range(n)], bias0=[base[ob:ob + nact]] * n, twin=[m ^ 1 for m in range(n)],
                      theta=theta, ref=S.ref_batch(nact), idx=idx)


MIXED_SCALE = np.array([0.02, -0.02, 0.0, 0.5, -0.1], F32)


@functools.lru_cache(maxsize=None)
def mixed_population():
    """five single members (set_members / eval_members: groups of one) on five windows of the ES table: +sigma, -sigma, 0 (theta itself:
    never an edge), and two scales of larger magnitude"""
    pop = es_population(KIND_ES, NACT)
    off = pop.idx[[0, 2, 4, 6, 8]]
    base = S.base_theta(KIND_ES, NACT)
    ob = pop.L.ob

    def theta(tab, m):
        return S.es_member_theta(KIND_ES, int(off[m]), float(MIXED_SCALE[m]), NACT, noise=tab)

    return Population("mixed", KIND_ES, NACT, S.TAP_STEPS, pop.table, S.tap_seeds(5), MIXED_SCALE,
                      entry0=[int(off[m]) + ob if MIXED_SCALE[m] != 0 else -1 for m in range(5)], bias0=[base[ob:ob + NACT]] * 5,
                      twin=[None] * 5, theta=theta, ref=S.ref_batch(NACT), off=off)


@functools.lru_cache(maxsize=None)
def ga_population(nact=NACT):
    """GAAtariPolicy: seven children of two parents, every root and every mutation on a window of its own.  (Fresh genomes have zeroed
    biases -- orc_ga_normc -- and cannot carry an edge: children only.)"""
    P = S.num_params(KIND_GA, nact)
    table = _randn(TABLE_SEED[KIND_GA, nact], 9 * P + 66)
    roots = (P + 3, 0)
    muts = [2 * P + 3 + 1, 3 * P + 8, 4 * P + 8, 5 * P + 8 + 2, 6 * P + 64, 7 * P + 64 + 1, table.size - P]      # the last legal slice among them
    chains = [(roots[i % 2], muts[i]) for i in range(7)]
    L = O.layout(O.KIND_GA, nact)

    def theta(tab, m):
        return O.ga_rebuild(L, tab, list(chains[m]), S.GA_SIGMA)

    return Population("ga", KIND_GA, nact, S.GA_TAP_STEPS, table, S.GA_SEEDS[1], [F32(S.GA_SIGMA)] * 7, entry0=[c[1] + L.ob for c in chains],
                      bias0=[np.zeros(nact, F32)] * 7, twin=[None] * 7, theta=theta, ref=None, chains=chains)


@functools.lru_cache(maxsize=None)
def large_population(nact=NACT):
    """LargeModel: six members -- a root and five children of two roots (powers 0.004 / 0.002), every seed on a window of its own"""
    from dne_hip import ga_gpu
    P = S.num_params(KIND_GA_LARGE, nact)
    sb = ga_gpu.model_scale_by(nact, KIND_GA_LARGE)
    table = _randn(TABLE_SEED[KIND_GA_LARGE, nact], 7 * P + 16)
    roots = ((0,), (P + 1,))
    muts = [2 * P + 1, 3 * P + 4, 4 * P + 6, 5 * P + 16, table.size - P]
    genomes = [roots[0]] + [roots[i % 2] + ((muts[i], 0.002 if i % 2 else 0.004),) for i in range(5)]
    L = O.layout(O.KIND_GA_LARGE, nact)

    def theta(tab, m):
        return O.ga_gpu_rebuild(tab, genomes[m], sb)

    bias0 = [(table[g[0]:g[0] + P][L.ob:L.ob + nact] * sb[L.ob:L.ob + nact]).astype(F32) for g in genomes]
    return Population("large", KIND_GA_LARGE, nact, S.LARGE_TAP_STEPS, table, S.tap_seeds(6), [F32(g[1][1]) if len(g) > 1 else F32(0) for g in genomes],
                      entry0=[g[1][0] + L.ob if len(g) > 1 else -1 for g in genomes], bias0=bias0, twin=[None] * 6, theta=theta, ref=None,
                      genomes=genomes, scale_by=sb)


# ---- construction ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base_rollouts(pop):
    """[m][t], t = 1..max(taps): the oracle's episode of every member on the unedited table, every step's logits"""
    steps = tuple(range(1, max(pop.taps) + 1))
    return [pop.rollout(pop.table, m, steps) for m in range(pop.n)]


def _bias(pop, m, b, x):
    return F32(pop.bias0[m][b] + F32(pop.scale[m] * F32(x)))


def _candidates(pop, T, m, picks):
    """(a, [b, ...]): the member's step-T top action and the columns b != a whose gap to the top is smaller at step T than at every earlier step
    (raising b flips step T first), never the twin's top at a step <= T nor the twin's own column; b < a first for about half the members,
    within a direction the smallest gap first"""
    base = _base_rollouts(pop)
    banned = set()
    tw = pop.twin[m]
    if tw is not None:
        banned |= set(base[tw][T]["actions"].tolist())
        if tw in picks:
            banned.add(picks[tw][1])
    acts = base[m][T]["actions"]
    a = int(acts[T - 1])
    gap = lambda t: np.float64(base[m][t]["logits"][acts[t - 1]]) - base[m][t]["logits"].astype(np.float64)
    earlier = np.min([gap(t) for t in range(1, T)], axis=0) if T > 1 else np.full(pop.nact, np.inf)
    g = gap(T)
    ok = [b for b in range(pop.nact) if b != a and b not in banned and g[b] < earlier[b]]
    below = ((m >> 1) ^ m) & 1 == 0                                 # members 0, 3, 4, 7, ...: b < a preferred; both signs of a pair's scale on both sides
    return a, sorted(ok, key=lambda b: ((b < a) != below, g[b]))


def _bisect(pop, m, T, a, b):
    """adjacent float32 (x_lo, x_hi) of the entry behind bias b between which the step-T decision flips a <-> b, or None when there is no such
    pair with logit_b exactly at logit_a on one side and one ulp from it on the other (one ulp of the entry, times the scale, can move the
    logit by two of ITS ulps past the tie)"""
    tap = _base_rollouts(pop)[m][T]
    w, bias, act, _ = pop.head_inputs(pop.table, m, tap)
    assert np.array_equal(head_logits(w, bias, act).view(np.int32), tap["logits"].view(np.int32)), (pop.name, m, T, "head_logits is not the oracle's head")
    x0 = pop.table[pop.entry0[m] + b]
    assert all(_bias(pop, m, c, pop.table[pop.entry0[m] + c]) == bias[c] for c in range(pop.nact)), (pop.name, m, "bias model")
    t, la = head_sums(w, act)[b], tap["logits"][a]

    def wins(x):
        lb = F32(t + _bias(pop, m, b, x))
        return bool(lb >= la) if b < a else bool(lb > la)

    sgn = 1.0 if pop.scale[m] > 0 else -1.0
    assert not wins(x0)
    d = max(abs((float(la) - float(t) - float(pop.bias0[m][b])) / float(pop.scale[m]) - float(x0)), 1e-3)
    for _ in range(60):
        x1 = F32(float(x0) + sgn * d)
        if wins(x1):
            break
        d *= 2.0
    else:
        return None
    k0, k1 = key(x0), key(x1)
    while abs(k1 - k0) > 1:
        mid = (k0 + k1) // 2
        if wins(unkey(mid)):
            k1 = mid
        else:
            k0 = mid
    if sorted(ulps(F32(t + _bias(pop, m, b, unkey(k))), la) for k in (k0, k1)) != [0, 1]:
        return None
    return unkey(min(k0, k1)), unkey(max(k0, k1))


class Case:
    """one (population, T): pos / vals["lo" | "hi"] (the entries that differ from the population's table), members[m] = dict(a, b, edge, tie_on, why),
    rollouts[which][m] (the oracle's T steps on that table) and heads[which][m] (head_inputs of step T)"""

    def table(self, which):
        t = self.pop.table.copy()
        t[self.pos] = self.vals[which]
        return t

    def describe(self, m, which):
        d = self.members[m]
        if d["a"] is None:
            return "member %d (no edited entry)" % m
        side = "not a knife-edge: %s" % d["why"] if not d["edge"] else "the exact tie" if d["tie_on"] == which else "the one-ulp side"
        return "member %d, a = %d, b = %d, scale %g, table '%s' (%s)" % (m, d["a"], d["b"], self.pop.scale[m], which, side)

    def edges(self):
        return [m for m in range(self.pop.n) if self.members[m]["edge"]]

    def counts(self):
        e = [self.members[m] for m in self.edges()]
        return dict(edges=len(e), members=self.pop.n, b_below_a=sum(d["b"] < d["a"] for d in e), b_above_a=sum(d["b"] > d["a"] for d in e),
                    tie_on_lo=sum(d["tie_on"] == "lo" for d in e), tie_on_hi=sum(d["tie_on"] == "hi" for d in e))


@functools.lru_cache(maxsize=None)
def _build_case(pop, T):
    c = Case()
    c.pop, c.T = pop, T
    picks, pos, lo, hi = {}, [], [], []
    for m in range(pop.n):
        if pop.entry0[m] < 0 or pop.scale[m] == 0 or _base_rollouts(pop)[m][T]["length"] != T:
            continue
        a, cols = _candidates(pop, T, m, picks)
        for b in cols:                                              # the first column that carries an exact edge; none: the member stays unedited
            r = _bisect(pop, m, T, a, b)
            if r is not None:
                picks[m] = (a, b)
                pos.append(pop.entry0[m] + b); lo.append(r[0]); hi.append(r[1])
                break
    c.pos = np.array(pos, np.int64)
    c.vals = dict(lo=np.array(lo, F32), hi=np.array(hi, F32))
    assert len(set(pos)) == len(pos) and all(x < y and ulps(x, y) == 1 for x, y in zip(lo, hi))
    # what counts is recomputed from the two final tables alone
    c.rollouts, c.heads = {}, {}
    for which in ("lo", "hi"):
        tab = c.table(which)
        c.rollouts[which] = [pop.rollout(tab, m, (T,))[T] for m in range(pop.n)]
        c.heads[which] = [pop.head_inputs(tab, m, c.rollouts[which][m]) for m in range(pop.n)]
    c.members = []
    for m in range(pop.n):
        if not picks.get(m):
            c.members.append(dict(a=None, b=None, edge=False, tie_on=None, why="no usable column"))
            continue
        a, b = picks[m]
        rl, rh = c.rollouts["lo"][m], c.rollouts["hi"][m]
        why, tie_on = None, None
        if not (rl["length"] == rh["length"] == T):
            why = "episode shorter than T"
        elif not np.array_equal(rl["actions"][:-1], rh["actions"][:-1]):
            why = "an earlier step moved"
        elif (int(rl["actions"][-1]), int(rh["actions"][-1])) != ((a, b) if pop.scale[m] > 0 else (b, a)):
            why = "step T does not flip a <-> b"
        else:
            d = {w: ulps(r["logits"][a], r["logits"][b]) for w, r in (("lo", rl), ("hi", rh))}
            bit_equal = {w: r["logits"][a].view(np.int32) == r["logits"][b].view(np.int32) for w, r in (("lo", rl), ("hi", rh))}
            if sorted(d.values()) != [0, 1] or not bit_equal[min(d, key=d.get)]:
                why = "logits %r / %r ulp apart on lo / hi" % (d["lo"], d["hi"])
            else:
                tie_on = min(d, key=d.get)
        c.members.append(dict(a=a, b=b, edge=why is None, tie_on=tie_on, why=why))
    return c


def case(pop, T):
    assert T in pop.taps
    return _build_case(pop, T)


# ---- the comparison the GPU tests and the CPU sensitivity test share -------------------------------------------------------------------------
def compare(c, run, ctx):
    """run(which) -> (returns [n], sign-returns [n], lengths [n], ram): the population evaluated for c.T steps on table `which` ("lo", then
    "hi") by an engine; ram [n][>= T][128] (every step's RAM; byte 38 is the action) or, GA kinds, [n][128] (the final RAM).  Every member
    must be the oracle's on both tables."""
    pop, T = c.pop, c.T
    for which in ("lo", "hi"):
        ret, sg, ln, ram = run(which)
        ret, sg, ln = np.asarray(ret).reshape(-1), np.asarray(sg).reshape(-1), np.asarray(ln).reshape(-1)
        for m in range(pop.n):
            want = c.rollouts[which][m]
            where = (ctx, "T = %d" % T, c.describe(m, which))
            assert ln[m] == T == want["length"], (where, "length", int(ln[m]))
            if pop.per_step_ram:
                assert np.array_equal(ram[m, :T], want["ram"]), (where, "actions (RAM byte 38) got / want", ram[m, :T, 38].tolist(), want["actions"].tolist())
            else:
                assert np.array_equal(ram[m], want["ram"][-1]), (where, "final RAM: last action (byte 38) got / want", int(ram[m, 38]), int(want["actions"][-1]))
            assert (ret[m], sg[m]) == (want["ret"], want["sign"]), (where, "return / sign-return", float(ret[m]), float(sg[m]), want["ret"], want["sign"])


def head_engine(c, head):
    """a CPU stand-in for compare(): the oracle's episode up to step T - 1, then step T's decision recomputed by `head` from the oracle's y3
    (y4) and bn of that step"""
    pop, T = c.pop, c.T

    def run(which):
        ret, sg, ln, rams = np.zeros(pop.n, F32), np.zeros(pop.n, F32), np.zeros(pop.n, np.int32), np.zeros((pop.n, T, O.RAM), np.uint8)
        for m in range(pop.n):
            want = c.rollouts[which][m]
            assert want["length"] == T
            env = O.WrappedEnv()
            env.reset(int(pop.seeds[m]))
            acts = want["actions"][:T - 1].tolist() + [head(*c.heads[which][m])]
            done = False
            for t, a in enumerate(acts):
                assert not done
                _, rew, done = env.step(a)
                ret[m] = F32(ret[m] + F32(rew)); sg[m] = F32(sg[m] + F32((rew > 0) - (rew < 0)))
                rams[m, t] = env.ram()
                ln[m] += 1
        return ret, sg, ln, rams if pop.per_step_ram else rams[:, T - 1]

    return run
