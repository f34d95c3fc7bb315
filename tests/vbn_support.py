"""TEST-ONLY helpers for the ModelVirtualBN engine kind (DNE_KIND_ES_VBN): the map from its flat vector onto the ES kind's, and the CPU
oracle behind the Engine surface for that kind.

ModelVirtualBN is, in real arithmetic, the ES network with every conv / fc bias at 0 and every BN gamma at 1, and the engine's contract for
the kind is exactly that network in the ES kind's fp32 order.  So the unchanged oracle (DNE_KIND_ES layout) checks it bit for bit on
expand(theta): w and out/b copied, each BatchNorm/b into its beta, +0.0f into conv1/conv2/fc biases, 1.0f into every gamma."""
import numpy as np

import oracle as O
from oracle_engine import OracleEngine

KIND_ES_VBN = 3   # DNE_KIND_ES_VBN (include/dne_hip.h)

# ModelVirtualBN tensor -> the ES kind's tensor that plays its part
TO_ES = {"layer1/conv1/w": "conv1/weights", "layer1/BatchNorm/b": "BatchNorm/beta",
         "layer2/conv2/w": "conv2/weights", "layer2/BatchNorm/b": "BatchNorm_1/beta",
         "layer3/fc/w": "fc/weights", "layer3/BatchNorm/b": "BatchNorm_2/beta",
         "layer4/out/w": "out/weights", "layer4/out/b": "out/biases"}
ZERO = ("conv1/biases", "conv2/biases", "fc/biases")
ONE = ("BatchNorm/gamma", "BatchNorm_1/gamma", "BatchNorm_2/gamma")


def layouts(nact):
    from dne_hip import _lib, policies
    return policies.flat_layout(_lib.KIND_ES_VBN, nact), policies.flat_layout(_lib.KIND_ES, nact)


def expand(theta, nact=18):
    """theta in the ModelVirtualBN layout -> the ES kind's vector of the same network"""
    (vspec, P), (espec, Pes) = layouts(nact)
    theta = np.asarray(theta, np.float32)
    assert theta.shape == (P,)
    out = np.full(Pes, np.nan, np.float32)
    for name, (off, shape) in vspec.items():
        eoff, eshape = espec[TO_ES[name]]
        n = int(np.prod(shape))
        assert n == int(np.prod(eshape))
        out[eoff:eoff + n] = theta[off:off + n]
    for name in ZERO + ONE:
        eoff, eshape = espec[name]
        out[eoff:eoff + int(np.prod(eshape))] = np.float32(0.0 if name in ZERO else 1.0)
    assert not np.isnan(out).any()
    return out


def contract(theta_es, nact=18):
    """the inverse of expand on its image"""
    (vspec, P), (espec, _) = layouts(nact)
    out = np.empty(P, np.float32)
    for name, (off, shape) in vspec.items():
        eoff, _ = espec[TO_ES[name]]
        n = int(np.prod(shape))
        out[off:off + n] = theta_es[eoff:eoff + n]
    return out


class OracleVBNEngine(OracleEngine):
    """OracleEngine for DNE_KIND_ES_VBN: theta, the noise slices, the weighted sum and the optimizer live in the native P; every member's
    perturbed vector is expanded and run through the oracle's ES network."""

    def __init__(self, n_actions=18, max_members=64, ref_count=16, **kw):
        super().__init__(O.KIND_ES, n_actions=n_actions, max_members=max_members, ref_count=ref_count, **kw)
        assert not self.bc_max_steps and not self.bc_final_only, "behaviour characterisations are not mirrored here"
        self.kind = KIND_ES_VBN
        self.P = layouts(n_actions)[0][1]
        self.theta = np.zeros(self.P, np.float32)

    def _oracle_theta(self, i):
        return expand(self._member_theta(i), self.n_actions)

    def _has_ref_pass(self):
        return True

    def es_eval(self, idx, sigma, tslimit, seeds, want_bc=False):
        assert not want_bc
        self.calls.append(("es_eval", len(idx)))
        n = len(idx)
        ret = np.zeros((n, 2), np.float32); sg = np.zeros((n, 2), np.float32); ln = np.zeros((n, 2), np.int32)
        for i in range(n):
            for s in range(2):
                th = expand(O.perturb(self.theta, self.noise, idx[i], sigma, 1 if s == 0 else -1), self.n_actions)
                ret[i, s], sg[i, s], ln[i, s] = O.rollout(self.L, th, self.ref, seeds[2 * i + s], tslimit)
        self._last = (np.asarray(idx, np.int64), ret, sg, ln)
        return ret, sg, ln

    def eval_members(self, n, tslimit, seeds, want_bc=False):
        assert not want_bc
        out = [O.rollout(self.L, expand(self._member_theta(i), self.n_actions), self.ref, seeds[i], tslimit) for i in range(n)]
        return (np.array([o[0] for o in out], np.float32), np.array([o[1] for o in out], np.float32),
                np.array([o[2] for o in out], np.int32))


def _vbn_pair(i):
    import oracle_pool
    noise, th, ref, idx, seeds, sigma, tslimit, nact, want_bc = oracle_pool._BASE
    L = O.layout(O.KIND_ES, nact)
    return [O.rollout(L, expand(O.perturb(th, noise, idx[i], sigma, 1 if s == 0 else -1), nact), ref, seeds[2 * i + s], tslimit,
                      want_bc=want_bc) for s in range(2)]


def es_pairs(noise, th, ref, idx, seeds, sigma, tslimit, nact=18, want_bc=False):
    """the oracle's rollouts of antithetic pairs around a ModelVirtualBN theta, over the host's cores (tests/oracle_pool.py): returns /
    sign-returns / lengths [n, 2] (+ the 2n RAM trajectories in member order).  seeds: 2 per pair."""
    import oracle_pool
    out = oracle_pool.pool_map(_vbn_pair, range(len(idx)), (noise, th, ref, np.asarray(idx, np.int64), seeds, sigma, tslimit, nact, want_bc))
    ret = np.array([[o[0][0], o[1][0]] for o in out], np.float32)
    sg = np.array([[o[0][1], o[1][1]] for o in out], np.float32)
    ln = np.array([[o[0][2], o[1][2]] for o in out], np.int32)
    bcs = [np.array(m[3]) for o in out for m in o] if want_bc else None
    return ret, sg, ln, bcs
