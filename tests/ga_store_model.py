"""TEST-ONLY: the GA store of csrc/engine.hip restated in Python over the CPU oracle, behind the Engine surface the store scenarios use
(tests/ga_store_support.py).  It lets the scenarios and check_generation run without a GPU (tests/test_ga_store_cpu.py), and it can be
built with one of the store's possible mistakes, so that the scenarios are shown to notice each:

  bug="sigma"   parents cached under one sigma are reused under another
  bug="bits"    the cache key leaves the power bits out
  bug="grow"    a slot the caller writes stays on the free list
  bug="stale"   a rebuild into a slot leaves the cache and the child slots pointing at it, and set_theta leaves it on the free list

Vectors are the oracle's own arithmetic (float32, one mutation after the other), so a correct model passes bit for bit."""
import numpy as np

import oracle as O
from dne_hip._lib import DneError
from ga_store_support import knobs_of, seeds_of
from oracle_engine import OracleEngine

_EPISODES = {}


def _episode(L, vec, seed, tslimit):
    key = (L.kind, hash(vec.tobytes()), int(seed), int(tslimit))
    if key not in _EPISODES:
        _EPISODES[key] = O.rollout(L, vec, None, seed, tslimit, want_bc=True)
    return _EPISODES[key]


class ModelStore(OracleEngine):
    def __init__(self, kind, n_actions=18, max_members=16, bug=None, **kw):
        super().__init__(kind, n_actions, max_members, 0)
        self.bug = bug
        self.mat, self.sort = knobs_of(kind)
        self.base_cap, self.free, self.cache, self.child_slots = 1, [], {}, []
        self.mode, self.cache_sigma = 0, np.float32(0)
        self.scale_by = None
        self.table = None            # (slot, off, scale, caller index) of the current members

    # ---- slots
    def _vec(self, slot):
        if slot == 0:
            return self.theta
        return self.bases.setdefault(slot, np.zeros(self.P, np.float32))

    def _grow(self, cap):
        for s in range(cap - 1, max(self.base_cap, 1) - 1, -1):
            self.free.append(s)
        self.base_cap = max(self.base_cap, cap)

    def _claim(self, slot, rebuild):
        if slot < 1:
            return
        if self.bug == "stale":
            if rebuild and slot in self.free:
                self.free.remove(slot)
            return
        if self.bug != "grow" and slot in self.free:
            self.free.remove(slot)
        if slot in self.child_slots:
            self.child_slots.remove(slot)
        self.cache = {k: s for k, s in self.cache.items() if s != slot}

    def set_theta(self, theta, slot=0):
        theta = np.array(theta, np.float32)
        if theta.size != self.P or slot < 0:
            raise DneError("set_theta")
        self._grow(slot + 1)
        self._claim(slot, False)
        if slot == 0:
            self.theta = theta
        else:
            self.bases[slot] = theta

    def get_theta(self, slot=0):
        if slot < 0 or slot >= self.base_cap:
            raise DneError("bad slot")
        return self._vec(slot).copy()

    def ga_set_init_scale(self, scale_by):
        self.scale_by = np.asarray(scale_by, np.float32)
        self.cache, self.child_slots = {}, []
        self.free = list(range(self.base_cap - 1, 0, -1))

    # ---- chains
    def _check_seed(self, s):
        if s < 0 or s + self.P > self.noise.size:
            raise DneError("noise index out of range")

    def _apply(self, v, seeds, powers):
        for s, p in zip(seeds, powers):
            v = (v + (np.float32(p) * self.noise[s:s + self.P]).astype(np.float32)).astype(np.float32)
        return v

    def _root(self, s0, powers_form):
        if powers_form:
            return (self.noise[s0:s0 + self.P] * self.scale_by).astype(np.float32)
        return O.ga_rebuild(self.L, self.noise, [s0], 0.0)

    def _rebuild(self, slot, seeds, powers, powers_form):
        if slot < 0 or len(seeds) < 1:
            raise DneError("bad arguments")
        self._grow(slot + 1)
        self._claim(slot, True)
        for s in seeds:
            self._check_seed(s)
        v = self._apply(self._root(seeds[0], powers_form), seeds[1:], powers)
        if slot == 0:
            self.theta = v
        else:
            self.bases[slot] = v
        return v.copy()

    def ga_rebuild(self, slot, seeds, sigma, copy_out=True):
        seeds = [int(s) for s in seeds]
        return self._rebuild(slot, seeds, [np.float32(sigma)] * (len(seeds) - 1), False)

    def ga_rebuild_powers(self, slot, genome, copy_out=True):
        if self.scale_by is None:
            raise DneError("dne_ga_set_init_scale first")
        return self._rebuild(slot, seeds_of(genome), [np.float32(g[1]) for g in genome[1:]], True)

    # ---- evaluation
    def ga_eval(self, chains, sigma, tslimit, env_seed, want_bc=False):
        return self._eval([[int(s) for s in c] for c in chains], None, np.float32(sigma), tslimit, env_seed, want_bc)

    def ga_eval_powers(self, genomes, tslimit, env_seed, want_bc=False):
        if self.scale_by is None:
            raise DneError("dne_ga_set_init_scale first")
        return self._eval([seeds_of(g) for g in genomes], [[np.float32(0)] + [np.float32(x[1]) for x in g[1:]] for g in genomes],
                          np.float32(0), tslimit, env_seed, want_bc)

    def _eval(self, chains, powers, sigma, tslimit, env_seed, want_bc):
        n = len(chains)
        if n < 1 or n > self.max_members:
            raise DneError("n out of range")
        pf = powers is not None

        def key_of(i, ln):
            if not pf:
                return tuple(chains[i][:ln])
            return tuple((chains[i][j], np.float32(powers[i][j]).tobytes() if j > 0 and self.bug != "bits" else b"") for j in range(ln))

        prefix, off, sc, spec = [], [], [], {}
        for i, c in enumerate(chains):
            if len(c) < 1:
                raise DneError("member %d has an empty seed chain" % i)
            for s in c:
                self._check_seed(s)
            ln = 1 if len(c) == 1 else len(c) - 1
            k = key_of(i, ln)
            prefix.append(k); off.append(c[-1])
            sc.append(np.float32(0) if len(c) == 1 else (powers[i][-1] if pf else sigma))
            spec.setdefault(k, (c[:ln], powers[i][1:ln] if pf else [sigma] * (ln - 1)))
        mode = 2 if pf else 1
        if self.mode != mode or (not pf and self.cache_sigma != sigma and self.bug != "sigma"):
            self.free += list(self.cache.values())
            self.cache = {}
            self.mode = mode
        self.cache_sigma = sigma
        needed = sorted(spec)
        fresh = [k for k in needed if k not in self.cache]
        if len(fresh) > len(self.free):
            self._grow(self.base_cap + len(fresh) - len(self.free))
        slot_of = {k: self.cache[k] for k in needed if k in self.cache}
        for k in fresh:
            s = self.free.pop()
            seeds, pw = spec[k]
            src = 0
            for m in range(len(k) - 1, 0, -1):
                if k[:m] in self.cache:
                    src = m
                    break
            v = self._vec(self.cache[k[:src]]).copy() if src else self._root(seeds[0], pf)
            self.bases[s] = self._apply(v, seeds[max(src, 1):], pw[max(src, 1) - 1:])
            slot_of[k] = s
        for k in [k for k in self.cache if k not in spec]:
            self.free.append(self.cache.pop(k))
        self.cache.update(slot_of)
        slot = [slot_of[k] for k in prefix]
        order = sorted(range(n), key=lambda i: slot[i]) if self.sort else list(range(n))
        pslot, poff, psc = [slot[i] for i in order], [off[i] for i in order], [sc[i] for i in order]
        if self.mat:
            if len(self.child_slots) < n:
                need = n - len(self.child_slots)
                if len(self.free) < need:
                    self._grow(self.base_cap + need - len(self.free))
                for _ in range(need):
                    self.child_slots.append(self.free.pop())
            for j in range(n):
                if psc[j] == 0.0:
                    continue
                cs = self.child_slots[j]
                self.bases[cs] = (self._vec(pslot[j]) + (psc[j] * self.noise[poff[j]:poff[j] + self.P]).astype(np.float32)).astype(np.float32)
                pslot[j], psc[j] = cs, np.float32(0)
        self.table = (np.array(pslot, np.int32), np.array(poff, np.int64), np.array(psc, np.float32), np.array(order, np.int32))
        self.members = self.table[:3]
        ret = np.zeros(n, np.float32); sg = np.zeros(n, np.float32); ln = np.zeros(n, np.int32); bc = np.zeros((n, 128), np.uint8)
        for j, i in enumerate(order):
            v = (self._vec(pslot[j]) + (psc[j] * self.noise[poff[j]:poff[j] + self.P]).astype(np.float32)).astype(np.float32)
            ret[i], sg[i], ln[i], bc[i] = _episode(self.L, v, env_seed[i], tslimit)
        return (ret, sg, ln, bc) if want_bc else (ret, sg, ln)

    def set_members(self, slot, off, scale):
        for s in np.asarray(slot):
            if s < 0 or s >= self.base_cap:
                raise DneError("base slot %d not allocated" % s)
        n = len(slot)
        self.table = (np.array(slot, np.int32), np.array(off, np.int64), np.array(scale, np.float32), np.arange(n, dtype=np.int32))
        self.members = self.table[:3]

    def _member_theta(self, i):
        slot, off, scale = self.members
        return (self._vec(int(slot[i])) + (np.float32(scale[i]) * self.noise[off[i]:off[i] + self.P]).astype(np.float32)).astype(np.float32)

    def debug_members(self):
        if self.table is None:
            return np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int32)
        return tuple(a.copy() for a in self.table)

    # ---- ES on the same engine (the LargeModel): antithetic pairs over slot 0, no reference batch
    def es_eval(self, idx, sigma, tslimit, seeds, want_bc=False):
        n = len(idx)
        ret = np.zeros((n, 2), np.float32); sg = np.zeros((n, 2), np.float32); ln = np.zeros((n, 2), np.int32)
        for i in range(n):
            for s in range(2):
                th = O.perturb(self.theta, self.noise, idx[i], sigma, 1 if s == 0 else -1)
                ret[i, s], sg[i, s], ln[i, s] = O.rollout(self.L, th, None, seeds[2 * i + s], tslimit)[:3]
        sl = np.zeros(2 * n, np.int32)
        self.set_members(sl, np.repeat(np.asarray(idx, np.int64), 2), np.tile(np.array([sigma, -sigma], np.float32), n))
        return ret, sg, ln
