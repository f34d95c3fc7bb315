"""TEST-ONLY: what a GA member is evaluated ON, held against the oracle over whole sequences of generations.

The GA store (csrc/engine.hip: ga_eval_impl, build_chain, grow_bases, dne_ga_rebuild*, dne_set_theta, dne_ga_set_init_scale) decides which
base slot holds which parent, which slots are free, which hold written-out children and which are the caller's.  Returns of short rollouts
say little about it: argmax actions over a few steps often agree for two different vectors.  Engine.debug_members() + get_theta(slot) give
the vector itself, all P floats: base[slot] + fl(scale * noise[off : off + P]), two float32 roundings (frames_support._expected).

  oracle_vector()      the bit-exact expectation: oracle.ga_rebuild (es_distributed genomes: normc root, one sigma) or oracle.ga_gpu_rebuild
                       (the GPU tree's genomes: scaled-noise root, one power per seed)
  f32_chain()          the sequential chain restated in numpy float32: v = v + fl(p * e)
  f64_chain()          the chain in float64 from the (bit-pinned) float32 root, and the element-wise bound a correct float32 chain keeps to it
  check_generation()   every member of an evaluated generation: vector, rollout, slot discipline, order, red zones
  scripted_generations(), special chains: the generations the GPU scenarios run, made without a GPU; store_model() counts what they do to
                       a parent cache (tests/test_ga_store_cpu.py holds the counts)

Genomes: form "sigma": a tuple of seeds (s0, s1, ...); form "powers": (s0, (s1, p1), (s2, p2), ...) as Engine.ga_eval_powers takes them."""
import functools

import numpy as np

import oracle as O
import step_tap_support as S
from step_tap_support import KIND_GA, KIND_GA_LARGE

NACT = 18
MAX_MEMBERS = 16
TSLIMIT = 6
SIGMA = 0.005
POWERS = (0.002, 0.004, -0.002, 0.001)          # per-seed powers of the scripted generations; one negative
CHAIN_CAP = 1024                                # build_chain's first buffer size: a chain of more mutations makes it regrow
U = 2.0 ** -24                                  # float32 unit roundoff


def noise_of(kind):
    return S.big_noise() if kind == KIND_GA_LARGE else S.small_noise()


def layout(kind):
    return O.layout(O.KIND_GA_LARGE if kind == KIND_GA_LARGE else O.KIND_GA, NACT)


@functools.lru_cache(maxsize=None)
def _noise64(kind):
    return noise_of(kind).astype(np.float64)


def last_offset(kind):
    """the last legal noise offset of a kind"""
    return noise_of(kind).size - S.num_params(kind, NACT)


@functools.lru_cache(maxsize=None)
def _scale_by(kind, which):
    from dne_hip import ga_gpu
    sb = ga_gpu.model_scale_by(NACT, kind)
    if which:                                   # another initial scale: 0.75 * the model's (exact in float32 up to one rounding, and nowhere equal)
        sb = (sb * np.float32(0.75)).astype(np.float32)
    sb.setflags(write=False)
    return sb


def scale_by(kind, which=0):
    """the per-parameter initial scale of the GPU tree's model (which = 0), or a different one (which = 1)"""
    return _scale_by(int(kind), int(which))


# ---- genomes ------------------------------------------------------------------------------------------------------------------------------
def seeds_of(genome):
    return [g[0] if isinstance(g, tuple) else g for g in genome]


def powers_of(genome, form, sigma):
    """the float32 factor of every mutation seed (genome[1:])"""
    if form == "sigma":
        return [np.float32(sigma)] * (len(genome) - 1)
    return [np.float32(g[1]) for g in genome[1:]]


def prefix_key(genome, form):
    """what the store keys a member's parent by: the genome without its last mutation (a root is its own parent); powers by their bits"""
    pre = genome if len(genome) == 1 else genome[:-1]
    if form == "sigma":
        return tuple(int(s) for s in pre)
    return (int(pre[0]),) + tuple((int(s), np.float32(p).tobytes()) for s, p in pre[1:])


def with_powers(chain, powers=POWERS):
    """a sigma-form chain as a powers-form genome, powers cycling through `powers`"""
    return (chain[0],) + tuple((s, powers[k % len(powers)]) for k, s in enumerate(chain[1:]))


# ---- reference vectors --------------------------------------------------------------------------------------------------------------------
def root_vector(kind, form, genome, sb=None):
    """the chain's start: normc(noise[s0]) (ga.py:256-260) or noise[s0] * scale_by (base.py:128-129), from the oracle"""
    noise = noise_of(kind)
    s0 = seeds_of(genome)[0]
    if form == "sigma":
        return O.ga_rebuild(layout(kind), noise, [s0], 0.0)
    return O.ga_gpu_rebuild(noise, (s0,), sb)


def oracle_vector(kind, form, genome, sigma=SIGMA, sb=None):
    """the genome's vector, bit for bit"""
    if form == "sigma":
        assert kind == KIND_GA
        return O.ga_rebuild(layout(kind), noise_of(kind), seeds_of(genome), sigma)
    return O.ga_gpu_rebuild(noise_of(kind), genome, sb)


def f32_chain(kind, form, genome, sigma=SIGMA, sb=None):
    """the sequential chain in numpy float32: v = v + fl(p * e), one mutation after the other"""
    noise, P = noise_of(kind), S.num_params(kind, NACT)
    v = root_vector(kind, form, genome, sb).copy()
    for s, p in zip(seeds_of(genome)[1:], powers_of(genome, form, sigma)):
        t = (np.float32(p) * noise[s:s + P]).astype(np.float32)
        v = (v + t).astype(np.float32)
    return v


def f64_chain(kind, form, genome, sigma=SIGMA, sb=None, block=1 << 16):
    """(value, bound): root + sum_k p_k * noise[s_k : s_k + P] in float64 from the float32 root, and the element-wise distance a float32
    chain of m products and m sequential additions may keep from it: 1.01 * (2m + 1) * 2^-24 * (|root| + sum_k |p_k * e_k|) -- every
    product carries one rounding (1 + d), every partial sum one more, so a term passes through at most m + 1 roundings and the root through
    m; (1 + u)^(m + 1) - 1 <= 1.01 (m + 1) u for m u < 0.01, and 2m + 1 is the issue's (looser) count.  Nothing measured."""
    noise, P = _noise64(kind), S.num_params(kind, NACT)          # (float32 -> float64 is exact)
    root = root_vector(kind, form, genome, sb).astype(np.float64)
    seeds = np.array(seeds_of(genome)[1:], np.int64)
    pw = np.array(powers_of(genome, form, sigma), np.float64)
    m = len(seeds)
    val, mag = root.copy(), np.abs(root)
    for lo in range(0, P, block):               # blocks of the vector stay in cache while every seed passes over them
        hi = min(lo + block, P)
        for s, p in zip(seeds, pw):
            t = p * noise[s + lo:s + hi]
            val[lo:hi] += t
            mag[lo:hi] += np.abs(t, out=t)
    return val, 1.01 * (2 * m + 1) * U * mag


def within_f64_bound(got, kind, form, genome, sigma=SIGMA, sb=None):
    """number of elements of `got` outside the float64 bound of the genome's chain"""
    val, bound = f64_chain(kind, form, genome, sigma, sb)
    return int((np.abs(got.astype(np.float64) - val) > bound).sum())


_ROLLOUTS, _BOUND_HELD = {}, {}


def oracle_vector_in_bound(kind, form, genome, sigma, sb_id, vector):
    """`vector` is the oracle's (the caller has compared it bit for bit): elements of it outside the float64 bound, worked out once per
    (genome, rules) and session"""
    key = (kind, form, genome, float(np.float32(sigma)) if form == "sigma" else None, sb_id if form == "powers" else None)
    if key not in _BOUND_HELD:
        _BOUND_HELD[key] = within_f64_bound(vector, kind, form, genome, sigma, scale_by(kind, sb_id) if form == "powers" else None)
    return _BOUND_HELD[key]


def oracle_rollout(kind, form, genome, sigma, sb_id, env_seed, tslimit, vector):
    """(return, sign-return, length, final RAM) of the oracle's episode on `vector`, computed once per (genome, rules, seed) and session"""
    key = (kind, form, genome, float(np.float32(sigma)) if form == "sigma" else None, sb_id if form == "powers" else None, int(env_seed), int(tslimit))
    if key not in _ROLLOUTS:
        r, s, l, ram = O.rollout(layout(kind), vector, None, env_seed, tslimit, want_bc=True)
        ram.setflags(write=False)
        _ROLLOUTS[key] = (r, s, l, ram)
    return _ROLLOUTS[key]


# ---- an evaluated generation against all of that -------------------------------------------------------------------------------------------
def knobs_of(kind):
    """(DNE_GA_MATERIALIZE, DNE_GA_SORT) as dne_create reads them under the current environment"""
    from dne_hip import _lib
    return _lib.debug_knob(kind, NACT, "DNE_GA_MATERIALIZE"), _lib.debug_knob(kind, NACT, "DNE_GA_SORT")


def member_vectors(engine):
    """every current member's effective vector, caller order: base[slot] + fl(scale * noise[off : off + P]) -> (vectors, slot, off, scale, who)"""
    noise, P = noise_of(engine.kind), engine.P
    slot, off, scale, who = engine.debug_members()
    bases = {int(s): engine.get_theta(int(s)) for s in np.unique(slot)}
    vec = [None] * len(slot)
    for j in range(len(slot)):
        t = (np.float32(scale[j]) * noise[off[j]:off[j] + P]).astype(np.float32)
        vec[int(who[j])] = (bases[int(slot[j])] + t).astype(np.float32)
    return vec, slot, off, scale, who


def check_generation(engine, genomes, form, sigma, results, env_seeds, tslimit, sb=None, sb_id=0, caller_slots=()):
    """Every caller genome i of the generation just evaluated (results = ga_eval* with want_bc): the vector it was evaluated on equals the
    oracle's rebuild bit for bit and keeps the float64 bound; (return, sign-return, length, final RAM) are the oracle's episode on that vector;
    the slots obey the store's rules; caller_index is a permutation (the identity under DNE_GA_SORT=0); no red zone is damaged.
    caller_slots: the base slots the caller wrote itself."""
    kind, n = engine.kind, len(genomes)
    mat, sort = knobs_of(kind)
    ret, sg, ln, ram = results
    vec, slot, off, scale, who = member_vectors(engine)
    assert len(slot) == n and sorted(who.tolist()) == list(range(n)), ("caller_index is no permutation", who.tolist(), n)
    if not sort:
        assert who.tolist() == list(range(n)), ("DNE_GA_SORT=0 keeps the caller's order", who.tolist())
    caller_slots = set(int(s) for s in caller_slots)
    by_prefix, by_slot, own = {}, {}, {}
    for j in range(n):
        i, g = int(who[j]), genomes[int(who[j])]
        sj, key = int(slot[j]), prefix_key(g, form)
        tag = "member %d (engine row %d, slot %d) %r" % (i, j, sj, g if len(g) < 6 else g[:2] + ("...%d seeds" % len(g),))
        want = oracle_vector(kind, form, g, sigma, sb)
        assert np.array_equal(vec[i], want), "%s: %d of %d elements are not the oracle's" % (tag, int((vec[i] != want).sum()), want.size)
        # (vec[i] IS want, bit for bit, so the bound is worked out on want, once per genome and session)
        assert oracle_vector_in_bound(kind, form, g, sigma, sb_id, want) == 0, tag + ": outside the float64 bound"
        r, s, l, oram = oracle_rollout(kind, form, g, sigma, sb_id, env_seeds[i], tslimit, want)
        assert (ret[i], sg[i], ln[i]) == (r, s, l), (tag, (ret[i], sg[i], ln[i]), (r, s, l))
        assert np.array_equal(ram[i], oram), tag + ": final RAM"
        assert sj != 0 and sj not in caller_slots, tag + ": evaluated out of slot 0 or a slot the caller wrote"
        mutated = len(g) > 1 and float(powers_of(g, form, sigma)[-1]) != 0.0
        if mat and mutated:                     # a written-out child: its own slot, the whole vector, no noise on top
            assert scale[j] == 0.0, tag + ": a materialised child carries a scale"
            assert sj not in own, tag + ": shares its child slot with member %d" % own.get(sj, -1)
            own[sj] = i
            continue
        assert by_prefix.setdefault(key, sj) == sj, tag + ": its parent sits in slot %d for another child" % by_prefix[key]
        assert by_slot.setdefault(sj, key) == key, tag + ": another parent shares its slot"
        last = seeds_of(g)[-1]
        assert int(off[j]) == last, (tag, "offset", int(off[j]), last)
        if len(g) == 1:
            assert scale[j] == 0.0, tag + ": a root carries a scale"
        elif not mat:
            p = powers_of(g, form, sigma)[-1]
            assert np.float32(scale[j]).tobytes() == np.float32(p).tobytes(), (tag, "scale", scale[j], p)
    assert not set(own) & set(by_slot), ("a child slot is a parent slot", sorted(set(own) & set(by_slot)))
    if sort and not mat:
        assert np.all(np.diff(slot) >= 0), ("DNE_GA_SORT=1 groups the members by parent slot", slot.tolist())
    assert engine.check_redzones() == 0


class Store:
    """One engine under test with what the caller wrote into it: run() evaluates a generation and checks it, then reads every caller-written
    slot back."""

    def __init__(self, engine, sb_id=None):
        self.e, self.kind = engine, engine.kind
        self.caller = {}                        # slot -> the vector the caller wrote
        self.sb_id, self.sb = None, None
        self.calls = 0
        if sb_id is not None:
            self.set_init_scale(sb_id)

    def set_init_scale(self, sb_id):
        self.sb_id, self.sb = sb_id, scale_by(self.kind, sb_id)
        self.e.ga_set_init_scale(self.sb)
        self.caller = {}                        # dne_ga_set_init_scale frees every slot but 0

    def evaluate(self, genomes, form, sigma=SIGMA, tslimit=TSLIMIT):
        self.calls += 1
        seeds = S.tap_seeds(MAX_MEMBERS * self.calls)[-len(genomes):]
        if form == "sigma":
            res = self.e.ga_eval([seeds_of(g) for g in genomes], sigma, tslimit, seeds, want_bc=True)
        else:
            res = self.e.ga_eval_powers(genomes, tslimit, seeds, want_bc=True)
        return res, seeds

    def run(self, genomes, form, sigma=SIGMA, tslimit=TSLIMIT):
        res, seeds = self.evaluate(genomes, form, sigma, tslimit)
        check_generation(self.e, genomes, form, sigma, res, seeds, tslimit, self.sb, self.sb_id, self.caller)
        self.check_caller_slots()
        return res

    def write(self, slot, genome, form, sigma=SIGMA):
        """ga_rebuild / ga_rebuild_powers of a genome into a slot of the caller's"""
        want = oracle_vector(self.kind, form, genome, sigma, self.sb)
        got = self.e.ga_rebuild(slot, seeds_of(genome), sigma) if form == "sigma" else self.e.ga_rebuild_powers(slot, genome)
        assert np.array_equal(got, want), ("rebuild into slot %d" % slot, genome)
        self.caller[slot] = want

    def write_theta(self, slot, vec):
        self.e.set_theta(vec, slot)
        if slot:
            self.caller[slot] = np.array(vec, np.float32)

    def check_caller_slots(self):
        for s, v in self.caller.items():
            got = self.e.get_theta(s)
            assert np.array_equal(got, v), "slot %d, written by the caller, lost %d of %d elements" % (s, int((got != v).sum()), v.size)

    def parent_snapshot(self):
        """{slot: vector} of every slot the current members read (parents, or written-out children)"""
        slot = self.e.debug_members()[0]
        return {int(s): self.e.get_theta(int(s)) for s in np.unique(slot)}


# ---- scripted generations -------------------------------------------------------------------------------------------------------------------
def scripted_generations(kind, form, n, T, gens, seed=2026):
    """`gens` Deep-GA generations of n members (ga.py:243-271 / the GPU tree's ga.py:161-166): generation 0 = n fresh roots; afterwards the
    best of the last generation unchanged (the elite) and n - 1 children of its top T, each its parent + one fresh seed.  Fitness is scripted
    (a fixed RandomState), the truncation is oracle.ga_select's.  Offsets include 0 and the last legal index, as roots and as mutations."""
    rs = np.random.RandomState(seed)
    hi = last_offset(kind)

    def fresh(k):
        return 0 if k == 0 else hi if k == 1 else int(rs.randint(0, hi + 1))

    def mutate(g, s):
        return g + ((s, POWERS[int(rs.randint(len(POWERS)))]) if form == "powers" else s,)

    pop = [(fresh(k),) for k in range(n)]
    out = [pop]
    for _ in range(1, gens):
        fitness = rs.randint(0, 50, len(pop)).astype(np.float32)
        top = [pop[i] for i in O.ga_select(fitness, T)]
        nxt = [top[0]]
        for k in range(n - 1):
            nxt.append(mutate(top[int(rs.randint(T))], fresh(k)))
        pop = nxt
        out.append(pop)
    return out


def store_model(generations, form):
    """What a parent cache does over these generations, counted without an engine: per generation the prefixes needed, how many of them are
    built fresh, from which cached prefix length each fresh one starts (0: from its root), how many cached parents are evicted, and whether
    an elite [.., s] sits next to its own children [.., s, t]."""
    cache, rows = set(), []
    for pop in generations:
        needed = {prefix_key(g, form) for g in pop}
        starts = []
        for key in sorted(needed - cache, key=repr):
            src = 0
            for k in range(len(key) - 1, 0, -1):
                if key[:k] in cache:
                    src = k
                    break
            starts.append(src)
        full = {prefix_key(g + (0,), "sigma") if form == "sigma" else prefix_key(g + ((0, 0.0),), form) for g in pop if len(g) > 1}
        rows.append(dict(needed=len(needed), fresh=len(needed - cache), starts=starts, evicted=len(cache - needed),
                         elite_with_children=len(full & needed)))
        cache = needed
    return rows


def block_chains(kind, form, seed=77):
    """Test 2's three calls.  Call 0 caches the root [p]; call 1 evaluates children of the parents [p, a, b], [p, a1..a8], [p, a1..a11] -- a
    prefix start ([p] is cached) followed by 2 seeds, one whole block of eight, one block and a tail of 3 in k_chain_sum; call 2 the same from
    the cached prefix [p, a, b] of length 3.  Powers differ per seed, one is negative."""
    rs = np.random.RandomState(seed)
    hi = last_offset(kind)
    pw = (0.002, -0.003, 0.0015, 0.004, 0.001, 0.0025, -0.0005, 0.003, 0.0035, 0.0005, 0.002)

    def ext(g, k):
        for j in range(k):
            s = int(rs.randint(0, hi + 1))
            g = g + ((s, pw[j % len(pw)]) if form == "powers" else s,)
        return g

    p = (int(rs.randint(0, hi + 1)),)
    call0 = [p, ext(p, 1)]
    pab = ext(p, 2)
    parents1 = [pab, ext(p, 8), ext(p, 11)]
    call1 = [ext(q, 1) for q in parents1 for _ in range(2)]
    parents2 = [ext(pab, 2), ext(pab, 8), ext(pab, 11)]
    call2 = [ext(q, 1) for q in parents2 for _ in range(2)] + [ext(pab, 1)]
    return call0, call1, call2


def long_genome(kind, form, mutations, seed=5):
    """one genome of `mutations` mutation seeds behind its root"""
    rs = np.random.RandomState(seed + mutations)
    hi = last_offset(kind)
    s = rs.randint(0, hi + 1, mutations + 1).tolist()
    return tuple(s) if form == "sigma" else with_powers(tuple(s))


# ---- the scenarios: the same calls on the HIP engine (tests/test_gpu_ga_store.py) and on the Python model of the store ----------------------
# make(kind) -> a fresh engine of that kind (max_members = MAX_MEMBERS, record_bc) with its noise table; the knobs come from the environment.
def _forms(st, form):
    if form == "powers":
        st.set_init_scale(0)
    return st


def scenario_generations(make, form, gens=8, n=12, T=3):
    """1: chains grow, parents are evicted, slots are recycled"""
    st = _forms(Store(make(KIND_GA)), form)
    for pop in scripted_generations(KIND_GA, form, n, T, gens):
        st.run(pop, form)
    return st


def scenario_large_generations(make):
    """1, LargeModel: three generations, and between two of them one ES step on slot 0 -- it must leave the GA's parents alone, and the GA
    must leave slot 0 as ES left it"""
    st = _forms(Store(make(KIND_GA_LARGE)), "powers")
    e, kind = st.e, KIND_GA_LARGE
    g = scripted_generations(kind, "powers", 6, 2, 3)
    st.run(g[0], "powers")
    st.run(g[1], "powers")
    before = st.parent_snapshot()
    th = oracle_vector(kind, "powers", (1_234_567,), sb=st.sb)
    idx = np.array([0, last_offset(kind)], np.int64)
    e.set_theta(th)
    ret, sg, ln = e.es_eval(idx, 0.02, TSLIMIT, S.tap_seeds(4))
    e.es_update(idx, ret, sg, "centered_rank", "adam", 0.005, 0.01)
    left = e.get_theta()
    _, want = O.Adam(th, 0.01).update(O.es_gradient(noise_of(kind), idx, ret, e.P), 0.005)
    assert np.array_equal(left, want), "the ES step on slot 0"
    for s, v in before.items():
        assert np.array_equal(e.get_theta(s), v), "the ES step changed base slot %d" % s
    st.run(g[2], "powers")
    assert np.array_equal(e.get_theta(), left), "a GA generation changed slot 0"
    return st


def scenario_blocks(make, form):
    """2: k_chain_sum from a cached prefix (src_len 1, then 3) over 2 seeds, one block of eight, a block and a tail of 3"""
    st = _forms(Store(make(KIND_GA)), form)
    for call in block_chains(KIND_GA, form):
        st.run(call, form)
    return st


def scenario_regrow(make, form):
    """3: 5 mutations, then CHAIN_CAP + 8 + 3 in one chain (the chain buffers regrow), then 5 again"""
    st = _forms(Store(make(KIND_GA)), form)
    for k, m in enumerate((5, CHAIN_CAP + 8 + 3, 5)):
        st.run([long_genome(KIND_GA, form, m + 1, seed=5 + k)], form)      # (m in the parent's chain, the last one applied on the fly)
    return st


def scenario_sigmas(make):
    """4: the same chains under sigma 0.005, 0.002, 0.005"""
    st = Store(make(KIND_GA))
    chains = scripted_generations(KIND_GA, "sigma", 8, 3, 3)[2]
    for sigma in (0.005, 0.002, 0.005):
        st.run(chains, "sigma", sigma)
    return st


def power_bit_genomes(chains):
    """parents that differ in one power only -- 0.002, the next float32 above it, -0.002 -- two children each"""
    p, a, t, t2 = chains[1][0], chains[2][1], chains[3][1], chains[4][1]
    up = float(np.nextafter(np.float32(0.002), np.float32(1)))
    parents = [(p, (a, 0.002)), (p, (a, up)), (p, (a, -0.002))]
    return [q + ((t, 0.001),) for q in parents] + [q + ((t2, 0.004),) for q in parents]


def scenario_forms(make):
    """5: sigma genomes, the same seed lists with powers, sigma again, powers under another initial scale; then power bits"""
    st = Store(make(KIND_GA))
    chains = scripted_generations(KIND_GA, "sigma", 8, 3, 3)[2]
    pg = [with_powers(c) for c in chains]
    st.run(chains, "sigma")
    st.set_init_scale(0)
    st.run(pg, "powers")
    st.run(chains, "sigma")
    st.set_init_scale(1)
    st.run(pg, "powers")
    genomes = power_bit_genomes(chains)
    assert len({prefix_key(g, "powers") for g in genomes}) == 3
    st.run(genomes, "powers")
    return st


def caller_chains(form):
    """the chains the caller rebuilds into slots 1..3 (1, 2 and 3 mutations; none of them a chain of the scripted generations)"""
    return [long_genome(KIND_GA, form, s, seed=300) for s in (1, 2, 3)]


def scenario_caller_slots(make, form):
    """6: slots the caller writes in the middle of a run stay the caller's, and the store does not go on reading them as its own"""
    import frames_support as F
    st = _forms(Store(make(KIND_GA)), form)
    e = st.e
    g = scripted_generations(KIND_GA, form, 8, 3, 3)
    st.run(g[1], form)                          # its parents -- with DNE_GA_MATERIALIZE its children too -- take the low slots
    st.run(g[2], form)
    for s, chain in enumerate(caller_chains(form), 1):
        st.write(s, chain, form)
    vec = oracle_vector(KIND_GA, "sigma", (4242, 777), 0.01)
    st.write_theta(4, vec)
    st.check_caller_slots()
    st.run(g[2], form)                          # the same children again: the cache is warm, and three of its slots are the caller's now
    bigger = scripted_generations(KIND_GA, form, 14, 6, 3, seed=99)[2]
    st.run(bigger, form)                        # more parents, 14 children: new slots are taken, the bases grow
    st.run(g[2], form)
    # the caller's slots under its own members (the frames_support pattern)
    slot = np.array([1, 2, 3, 4], np.int32)
    off = np.array([0, last_offset(KIND_GA), 123_457, 2_000_001], np.int64)
    scale = np.array([0.02, -0.02, 0.0, 0.5], np.float32)
    frames = np.ascontiguousarray(F.frames()[[0, 1, 3, 21]])
    e.set_members(slot, off, scale)
    who = e.debug_members()[3]
    assert who.tolist() == [0, 1, 2, 3]
    e.env_set_observation(frames)
    actions, logits = e.act(4)
    L, noise = layout(KIND_GA), noise_of(KIND_GA)
    for i in range(4):
        th = (st.caller[int(slot[i])] + (scale[i] * noise[off[i]:off[i] + e.P]).astype(np.float32)).astype(np.float32)
        a, lg = O.act(L, th, None, frames[i])
        assert np.array_equal(logits[i], lg) and int(actions[i]) == int(a), "act on the caller's slot %d" % slot[i]
    st.check_caller_slots()
    assert e.check_redzones() == 0
    return st


def _children(form, parents, n, seed):
    """n children, child k of parents[k % len(parents)], each with one fresh seed (powers form: a power of POWERS)"""
    rs = np.random.RandomState(seed)
    hi = last_offset(KIND_GA)
    out = []
    for k in range(n):
        s = int(rs.randint(0, hi + 1))
        out.append(parents[k % len(parents)] + ((s, POWERS[k % len(POWERS)]) if form == "powers" else s,))
    return out


def four_parent_generation(form):
    roots = [(r,) for r in (17, 1_000_000, 2_222_222, last_offset(KIND_GA))]
    return _children(form, _children(form, roots, 4, 31), 8, 32)


def scenario_caller_slot_first(make, form):
    """6, the mirror: set_theta(3) on a fresh engine grows the bases past slot 3; an evaluation with four parents must not take slot 3"""
    st = _forms(Store(make(KIND_GA)), form)
    vec = oracle_vector(KIND_GA, "sigma", (4242, 777), 0.01)
    st.write_theta(3, vec)
    pop = four_parent_generation(form)
    assert len({prefix_key(x, form) for x in pop}) == 4
    st.run(pop, form)
    return st


def growth_generations(form):
    """7: (small, big): 4 children of 2 parents; 14 children of 7 parents, the two among them"""
    roots = [(r,) for r in (5, 400_001, 800_002, 1_200_003, 1_600_004, 2_000_005, 2_400_006)]
    parents = _children(form, roots, 7, 51)
    return _children(form, parents[:2], 4, 52), _children(form, parents, 14, 53)


def scenario_growth(make, form):
    """7: n = 4 -> 14 -> 4 -> 14 with 2 -> 7 -> 2 -> 7 parents: slot 0, the caller's slot and the cached parents keep their contents whenever the bases grow"""
    st = _forms(Store(make(KIND_GA)), form)
    e = st.e
    v0 = oracle_vector(KIND_GA, "sigma", (31_337,), 0.0)
    e.set_theta(v0)
    st.write_theta(2, oracle_vector(KIND_GA, "sigma", (4242, 777), 0.01))
    small, big = growth_generations(form)
    mat = knobs_of(KIND_GA)[0]
    def parent_slots(pop):                      # without DNE_GA_MATERIALIZE the members' slots are their parents' slots
        sl, _, _, who = e.debug_members()
        return {prefix_key(pop[int(who[j])], form): int(sl[j]) for j in range(len(sl))}

    last = None
    for pop in (small, big, small, big):
        before = st.parent_snapshot()
        held = parent_slots(last) if last and not mat else {}
        st.run(pop, form)
        last = pop
        assert np.array_equal(e.get_theta(0), v0), "slot 0 changed"
        if not mat:
            now = parent_slots(pop)
            for key, s in held.items():
                if key in now:                  # a parent both generations need: the same slot, the same contents, no rebuild
                    assert now[key] == s, "a cached parent moved from slot %d to %d" % (s, now[key])
                    assert np.array_equal(e.get_theta(s), before[s]), "cached parent in slot %d changed" % s
    return st


def scenario_duplicates(make, form):
    """8: the same child twice; a root that is a member and a parent; an elite [p, s] next to its own children [p, s, t]"""
    st = _forms(Store(make(KIND_GA)), form)
    hi = last_offset(KIND_GA)
    p, q = 1_000_003, hi
    m = (lambda s, w=0.002: (s, w)) if form == "powers" else (lambda s, w=None: s)
    s, t, t2, u, w = m(77), m(0, -0.002), m(hi, 0.004), m(2_000_000), m(555_555, 0.001)
    first = [(p,), (p, s), (p, s), (p, s, t), (p, s, t2), (p, u), (q,), (q, s), (p, s, t)]
    st.run(first, form)
    second = [(p, s, t), (p, s, t, w), (p, s, t, u), (p, s, t, w), (p,), (p, s)]   # the elite's children start from the cached [p, s]
    st.run(second, form)
    return st


def scenario_refusals(make, form):
    """9: calls the engine refuses in the middle of a run leave the store as it was"""
    from dne_hip._lib import DneError
    st = _forms(Store(make(KIND_GA)), form)
    e = st.e
    g = scripted_generations(KIND_GA, form, 8, 3, 4)
    st.run(g[0], form)
    st.run(g[1], form)
    before = st.parent_snapshot()
    table = [a.copy() for a in e.debug_members()]
    past = last_offset(KIND_GA) + 1
    bad = [g[2][:3] + [()] + g[2][3:],                                                        # an empty chain
           g[2][:5] + [g[2][5] + ((past, 0.002) if form == "powers" else past,)] + g[2][6:],  # one seed past the table
           (g[2] * 3)[:MAX_MEMBERS + 1]]                                                      # more members than the engine has
    for pop in bad:
        try:
            st.evaluate(pop, form)
        except DneError:
            pass
        else:
            raise AssertionError("not refused: %d members" % len(pop))
        for s, v in before.items():
            assert np.array_equal(e.get_theta(s), v), "a refused call changed base slot %d" % s
        assert all(np.array_equal(a, b) for a, b in zip(table, e.debug_members())), "a refused call changed the member table"
    st.run(g[2], form)
    return st
