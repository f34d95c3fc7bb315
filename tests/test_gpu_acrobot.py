"""GPU: gym.Acrobot-v1 on the device (DNE_ENV_ACROBOT: csrc/acrobot.h inside k_dense_run<9>, k_stepenv_reset_acrobot / _step_acrobot, k_dense_bc<9>
and the D = 4 novelty kernels) against the host twins.  Both sides are the same text with contraction off, so every comparison is bit for bit:
whole episodes through dne_eval_members and dne_es_eval, the step-at-a-time batch, the policy behind the batch, the GA bank and both novelty
forms over final states, and two drivers row by row against AcrobotHostEngine.  DESIGN.md section 19."""
import numpy as np
import pytest

import acrobot_support as A
import dense_support as D

pytestmark = pytest.mark.gpu
M = 68
SHAPE_IDS = ["x".join(str(w) for w in s[0]) or "linear" for s in A.SHAPES]


def _members(hidden, n, sigma, extra=None):
    """n member descriptors over base slots 0 and 1 (+-sigma, offsets up to the table's last admissible one); without hidden layers member 0 is
    the solving member and member 1 the all-zero one (slots 2 and 3 at scale 0) and every third member a perturbed solving one, so that
    workgroups leave the loop at different steps; with hidden layers member 1 is the all-zero one.  -> (slot, off, scale, extra thetas for slots 2.., the members' thetas)"""
    P = A.num_params(hidden)
    tab, bases = D.noise(), A.base_thetas(hidden)
    last = tab.size - P
    slot = (np.arange(n) % 2).astype(np.int32)
    off = ((np.arange(n, dtype=np.int64) * 7919 + 13) % (last + 1)).astype(np.int64)
    off[-1] = last
    scale = np.where(np.arange(n) % 4 < 2, sigma, -sigma).astype(np.float32)
    if extra is None:
        extra = [A.solver_theta(), A.zero_theta(P)] if not hidden else [np.zeros(P, np.float32)] * 2
    for k in range(min(n, 2)):
        if hidden and k == 0:
            continue
        slot[k], off[k], scale[k] = 2 + k, 0, 0.0
    if not hidden:
        slot[3::3] = 2                                                      # every third member is the solving one, perturbed: it ends early, at a step of its own
    slots = list(bases) + extra
    th = np.stack([(slots[s] + np.float32(c) * tab[o:o + P]).astype(np.float32) for s, o, c in zip(slot, off, scale)])
    return slot, off, scale, extra, th


# ---- 1. whole episodes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", A.SHAPES, ids=SHAPE_IDS)
def test_whole_episodes_equal_the_twin(shape):
    hidden, nl = shape
    e = A.device_engine(hidden, nl, M)
    try:
        P, tab = e.P, D.noise()
        bases = A.base_thetas(hidden)
        e.set_theta(bases[0], 0); e.set_theta(bases[1], 1)
        spread = 0
        for sigma in (0.0, 0.05):
            for n in (1, 5, 67):
                slot, off, scale, extra, th = _members(hidden, n, sigma)
                e.set_theta(extra[0], 2); e.set_theta(extra[1], 3)
                seeds = (np.arange(n, dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32)
                pairs = (n + 1) // 2
                idx = ((np.arange(pairs, dtype=np.int64) * 104729 + 7) % (tab.size - P + 1)).astype(np.int64)
                idx[-1] = tab.size - P
                th2 = np.stack([(bases[0] + np.float32(s) * tab[i:i + P]).astype(np.float32) for i in idx for s in (sigma, -sigma)])
                seeds2 = (np.arange(2 * pairs, dtype=np.uint64) * 40503 + 2 ** 31).astype(np.uint32)
                for tslimit in (1, 7, 500):
                    want = A.rollout(th, hidden, nl, seeds, tslimit)
                    e.set_members(slot, off, scale)
                    ret, sg, ln = e.eval_members(n, tslimit, seeds)
                    assert A.same(ln, want["lengths"]) and A.same(ret, want["returns"]) and A.same(sg, want["signreturns"]), (sigma, n, tslimit)
                    assert A.same(e.dense_final_state(n), want["state"]), (sigma, n, tslimit)
                    if tslimit == 500 and n == 67:
                        spread = max(spread, len(set(ln.tolist())))
                    want = A.rollout(th2, hidden, nl, seeds2, tslimit)
                    ret, sg, ln = e.es_eval(idx, sigma, tslimit, seeds2)
                    assert A.same(ln.reshape(-1), want["lengths"]) and A.same(ret.reshape(-1), want["returns"]), (sigma, n, tslimit)
                    assert A.same(sg.reshape(-1), want["signreturns"]) and A.same(e.dense_final_state(2 * pairs), want["state"]), (sigma, n, tslimit)
        if not hidden:
            assert spread >= 3                                              # the solving member, the all-zero member, the rest: different last steps
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- 2. the step-at-a-time batch ---------------------------------------------------------------------------------------------------------------------
def _same_batch(e, h, idx, nan=False):
    same = A.same_nan if nan else A.same
    (s1, t1, d1), (s2, t2, d2) = e.stepenv_state(idx), h.stepenv_state(idx)
    return same(s1, s2) and A.same(t1, t2) and A.same(d1, d2) and same(e.stepenv_observation(idx), h.stepenv_observation(idx))


def test_step_at_a_time_batch():
    from dne_hip import _lib
    e, h = A.device_engine((), "relu", 8), A.host_engine((), "relu", 8)
    try:
        allidx = np.arange(7, dtype=np.int32)
        seeds = np.array([0, 2 ** 31, 2 ** 32 - 1, 1, 2, 3, 4], np.uint32)
        for x in (e, h):
            x.stepenv_reset(allidx, seeds, 9)
        assert _same_batch(e, h, allidx) and A.same(e.stepenv_state([0])[0][0], np.array(A.SEED0_STATE))
        rs = np.random.RandomState(3)
        for t, idx in enumerate(([6, 2, 4], [0, 1, 2, 3, 4, 5, 6], [5], [3, 0], [1, 6, 5, 4, 3, 2, 0], [2, 4, 6], [0, 1, 2, 3, 4, 5, 6])):
            idx = np.array(idx, np.int32)
            acts = rs.randint(0, 3, idx.size).astype(np.int32)
            (r1, d1), (r2, d2) = e.stepenv_step(acts, idx), h.stepenv_step(acts, idx)
            assert A.same(r1, r2) and A.same(d1, d2) and _same_batch(e, h, allidx), t
        # hand-placed states through set_state: the threshold, +-pi, the clamps, NaN; every action; the environments the list leaves out keep every bit
        placed = list(A.threshold_states().values()) + A.edge_states()
        for a in range(3):
            for k in range(0, len(placed), 5):
                part = np.array(placed[k:k + 5], np.float64)
                idx = np.array([6, 1, 3, 0, 5][:len(part)], np.int32)
                for x in (e, h):
                    x.stepenv_set_state(part, np.zeros(len(part), np.int32), idx)
                assert _same_batch(e, h, allidx, nan=True)
                (r1, d1), (r2, d2) = e.stepenv_step(np.full(len(part), a, np.int32), idx), h.stepenv_step(np.full(len(part), a, np.int32), idx)
                assert A.same(r1, r2) and A.same(d1, d2) and _same_batch(e, h, allidx, nan=True), (a, k)
        # a done environment stepped again keeps every bit and earns 0
        for x in (e, h):
            x.stepenv_reset(allidx, seeds, 2)
        for t in range(2):
            r1, d1 = e.stepenv_step(np.full(7, 2, np.int32), allidx)
        assert d1.all() and r1.tolist() == [-1.0] * 7
        before = (e.stepenv_state(allidx), e.stepenv_observation(allidx))
        r1, d1 = e.stepenv_step(np.zeros(7, np.int32), allidx)
        after = (e.stepenv_state(allidx), e.stepenv_observation(allidx))
        assert r1.tolist() == [0.0] * 7 and d1.all() and all(A.same(a, b) for a, b in zip(before[0], after[0])) and A.same(before[1], after[1])
        # refusals, the batch unchanged
        with pytest.raises(_lib.DneError, match="action 3 at position 1, Acrobot-v1 has actions 0, 1 and 2"):
            e.stepenv_step(np.array([0, 3], np.int32), np.array([0, 1], np.int32))
        with pytest.raises(_lib.DneError, match="takes int32 actions"):
            e.stepenv_step(np.zeros(2, np.float32), np.array([0, 1], np.int32), as_int=False)
        with pytest.raises(_lib.DneError, match="seeds is NULL"):
            e.stepenv_reset(allidx, None)
        assert all(A.same(a, b) for a, b in zip(e.stepenv_state(allidx), after[0])) and e.check_redzones() == 0
    finally:
        e.close()


# ---- 3. the policy on the batch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", A.SHAPES, ids=SHAPE_IDS)
def test_policy_on_the_batch(shape):
    from dne_hip import _lib
    hidden, nl = shape
    n = 7
    e = A.device_engine(hidden, nl, 8)
    try:
        bases = A.base_thetas(hidden)
        e.set_theta(bases[0], 0); e.set_theta(bases[1], 1)
        knife = None
        if not hidden:                                                     # the argmax's edge: a tie of three, a tie of two behind a smaller logit
            knife = [A.zero_theta(), A.zero_theta()]
            knife[1][-3:] = (1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), np.nextafter(np.float32(1.0), np.float32(2.0)))
        slot, off, scale, extra, th = _members(hidden, n, 0.05, knife)
        e.set_theta(extra[0], 2); e.set_theta(extra[1], 3)
        e.set_members(slot, off, scale)
        seeds = np.arange(n, dtype=np.uint32) + 5
        whole = A.rollout(th, hidden, nl, seeds)
        allidx = np.arange(n, dtype=np.int32)
        e.stepenv_reset(allidx, seeds)
        obs = e.stepenv_observation(allidx)
        out, act = e.stepenv_act(n=n)
        _, want_out, want_act = _lib.dense_forward_host(th, obs, A.ENV, hidden, nl, 3)
        assert out.shape == (n, 3) and A.same(out, want_out) and act.dtype == np.int32 and A.same(act, want_act)
        if not hidden:
            assert act[:2].tolist() == [0, 1]
        idx, mem = np.array([4, 0, 6], np.int32), np.array([1, 1, 5], np.int32)     # a permutation, one member twice
        out, act = e.stepenv_act(idx, mem)
        _, want_out, want_act = _lib.dense_forward_host(th[mem], obs[idx], A.ENV, hidden, nl, 3)
        assert A.same(out, want_out) and A.same(act, want_act)
        # in rounds of 1, 3 and to the end: one whole-episode evaluation
        total, steps = np.zeros(n, np.float64), np.zeros(n, np.int32)
        for rounds in (1, 3, 1000):
            rew, took, done = e.stepenv_run(rounds, allidx)
            total += rew.astype(np.float64); steps += took
            assert np.all(took <= rounds)
        assert done.all() and A.same(steps, whole["lengths"]) and A.same(total.astype(np.float32), whole["returns"])   # integer rewards: the split is exact
        state, t, dn = e.stepenv_state(allidx)
        assert A.same(state, whole["state"]) and A.same(t, whole["lengths"]) and dn.all()
        ret, _, ln = e.eval_members(n, 500, seeds)
        assert A.same(ret, whole["returns"]) and A.same(ln, whole["lengths"]) and A.same(e.dense_final_state(n), whole["state"])
        assert A.same(e.stepenv_state(allidx)[0], state)                    # a whole-episode evaluation leaves the batch as it was
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- 4. the GA bank and novelty over final states ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", ((), (16, 16)), ids=("P21", "P435"))
def test_ga_bank_two_generations(hidden):
    from dne_hip import policies
    e, h = A.device_engine(hidden, "relu", 16), A.host_engine(hidden, "relu", 16)
    try:
        P, count = e.P, D.noise().size
        assert P == (435 if hidden else 21)
        sb = policies.dense_scale_by(A.ENV, hidden, 3)
        last = count - P
        genomes = [(100,), (200, (last, 0.02)), (5, (6, 0.02), (7, -0.01))]
        rs = np.random.RandomState(P)
        for x in (e, h):
            x.dense_ga_set_init_scale(sb)
            x.dense_ga_build(genomes)
        for gen in range(2):
            n = 9
            parent = np.array([0, 1, 2, 0, 1, 2, -1, 2, -1], np.int32)       # children of every parent, and two roots
            idx = rs.randint(0, last + 1, n).astype(np.int64); idx[3] = last
            power = np.full(n, 0.02, np.float32)
            seeds = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
            for tslimit in (7, 500):
                got, want = e.dense_ga_eval(parent, idx, power, tslimit, seeds), h.dense_ga_eval(parent, idx, power, tslimit, seeds)
                assert all(A.same(a, b) for a, b in zip(got, want)) and A.same(e.dense_final_state(n), h.dense_final_state(n)), (gen, tslimit)
            keep = np.array([4, 0, 7], np.int32)                              # two children and, in the kept form, parent 1 itself
            p2, i2, w2 = parent[keep].copy(), idx[keep].copy(), power[keep].copy()
            p2[1], i2[1] = 1, -1
            for x in (e, h):
                x.dense_ga_promote(p2, i2, w2)
            assert e.dense_ga_parents() == 3 and all(A.same(e.dense_ga_get_parent(j), h.bank[j]) for j in range(3)), gen
        assert e.check_redzones() == 0
    finally:
        e.close()


def test_novelty_over_final_states():
    from dne_hip import _lib
    e = A.device_engine((), "relu", 16)
    try:
        n = 9
        bases = A.base_thetas(())
        e.set_theta(bases[0], 0); e.set_theta(bases[1], 1)
        slot, off, scale, extra, th = _members((), n, 0.05)
        e.set_theta(extra[0], 2); e.set_theta(extra[1], 3)
        e.set_members(slot, off, scale)
        seeds = np.arange(n, dtype=np.uint32) + 50
        e.eval_members(n, 500, seeds)
        rec = e.dense_final_state(n)
        bc = e.dense_bc(n)
        assert e.dense_bc_dim() == 4 and bc.shape == (n, 4) and A.same(bc, rec.astype(np.float32)) and A.same(bc, _lib.dense_bc_host(A.ENV, rec))
        rs = np.random.RandomState(9)
        pts = rs.uniform(-3, 3, (9, 4)).astype(np.float32)
        for narch in (0, 1, 9):
            e.dense_archive_clear()
            if narch:
                e.dense_archive_append(pts[:narch])
            assert e.dense_archive_size() == narch
            for k in (1, 3):
                assert A.same(np.asarray(e.dense_novelty_pool(k, n=n)), _lib.dense_novelty_pool_host(bc, pts[:narch], k)), (narch, k)
                if narch:
                    assert A.same(np.asarray(e.dense_novelty(k, n=n)), _lib.dense_novelty_host(bc, pts[:narch], k)), (narch, k)
                else:
                    with pytest.raises(_lib.DneError):
                        e.dense_novelty(k, n=n)
        e.dense_archive_append_members(np.array([1, 4, 7], np.int32))
        assert A.same(e.dense_archive(), np.concatenate([pts, bc[[1, 4, 7]]]))
        assert A.same(np.asarray(e.dense_novelty(3, n=n)), _lib.dense_novelty_host(bc, e.dense_archive(), 3))
        assert e.check_redzones() == 0
    finally:
        e.close()


# ---- 5. the drivers against the CPU ----------------------------------------------------------------------------------------------------------------------
def test_es_driver_on_the_device_equals_the_host_engine(tmp_path):
    """es_gpu.main on an engine the driver opens itself (SimpleClassifier: hidden (16, 16), relu) against the same run on AcrobotHostEngine"""
    from dne_hip import es_gpu
    exp = A.es_exp("SimpleClassifier")
    a = es_gpu.main(str(tmp_path / "hip"), engine=None, noise=D.shared_noise(), seed=4, max_iters=2, **exp)
    b = es_gpu.main(str(tmp_path / "host"), engine=A.host_engine((16, 16), "relu", 16), noise=D.shared_noise(), seed=4, max_iters=2, **exp)
    assert a.it == b.it == 2 and a.game == b.game == A.GAME and a.model == b.model == "SimpleClassifier" and a.num_params == 435
    assert D.same_rows(D.log_rows(tmp_path / "hip"), D.log_rows(tmp_path / "host")) and len(D.log_rows(tmp_path / "hip")) == 2
    assert A.same(a.theta, b.theta) and A.same(a.optimizer[0], b.optimizer[0]) and A.same(a.optimizer[1], b.optimizer[1])
    assert (a.timesteps_so_far, a.num_frames) == (b.timesteps_so_far, b.num_frames)


def test_ga_ns_driver_on_the_device_equals_the_host_engine(oracle, tmp_path):
    from dne_hip import ga_gpu
    exp = A.ga_exp("LinearClassifier", novelty_search={"k": 3, "archive_prob": 0.5})
    host = A.host_engine((), "relu", 16)
    a = ga_gpu.dense_ns_main(str(tmp_path / "hip"), engine=None, noise=D.shared_noise(), seed=4, max_iters=2, **exp)
    b = ga_gpu.dense_ns_main(str(tmp_path / "host"), engine=host, noise=D.shared_noise(), seed=4, max_iters=2, **exp)
    (ta, va, sa), (tb, vb, sb) = a, b
    assert (ta, va) == (tb, vb) and sa.it == sb.it == 2 and sa.game == A.GAME and sa.model == "LinearClassifier" and sa.num_params == 21
    assert [o.seeds for o in sa.population] == [o.seeds for o in sb.population] and [o.rewards for o in sa.population] == [o.rewards for o in sb.population]
    assert [o.novelty for o in sa.population] == [o.novelty for o in sb.population] and A.same(sa.archive, sb.archive) and len(sa.archive) > 0
    assert D.same_rows(D.log_rows(tmp_path / "hip"), D.log_rows(tmp_path / "host")) and len(D.log_rows(tmp_path / "hip")) == 2
