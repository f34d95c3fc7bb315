"""TEST-ONLY: the reference batches of the unique-operand reference pass (csrc/ref_index.h) and the numpy side of its index:
tests/test_ref_index_cpu.py (the index against numpy) and tests/test_gpu_ref_dedup.py (the pass against the oracle, bit for bit); the
route of the reference pass (dedup or dense) as something a test sets, asserts and prints (route_env, expect_route)."""
import numpy as np

N1, N2 = 441, 121
ROUTE_FS = (16, 32, 64, 128)          # the reference counts at which the engine may take the dedup route (engine.hip: ref_default_route)
ROUTES = ("default", "dense")         # "default": the route dne_set_ref_batch picks per batch; "dense": DNE_REF_DEDUP=0, the dense kernels


def routes(F):
    """the routes a reference-pass test runs at F frames: both where the engine has two, one elsewhere"""
    return ROUTES if F in ROUTE_FS else ROUTES[:1]


def route_id(route):
    """suffix of a parametrised test id: the default route keeps the id the case had before it had a route"""
    return "" if route == "default" else "-" + route


def route_env(monkeypatch, route):
    """Call BEFORE the engine is made (dne_create reads the knobs once).  "dense" sets DNE_REF_DEDUP=0; "default" leaves the environment
    alone, so a suite run under DNE_REF_DEDUP=0 by hand takes the dense kernels everywhere.  Returns the knob's value for expect_route."""
    from dne_hip import _lib
    assert route in ROUTES, route
    if route == "dense":
        monkeypatch.setenv("DNE_REF_DEDUP", "0")
    return _lib.debug_knob(_lib.KIND_ES, 18, "DNE_REF_DEDUP")


def expect_route(engine, ref, knob, want_dedup=None):
    """Call after every set_ref_batch(ref).  knob: DNE_REF_DEDUP as the engine was created (route_env).  With the knob on and F in
    ROUTE_FS the engine's route and U1 / U2 must be the host's (dne_debug_ref_index: the verdict of ref_dedup_pays, no device), and the
    route a test's table names for the batch (want_dedup) must be that route; with the knob off, or at any other F, the route is the dense
    one and the engine reports U1 = U2 = 0.  Returns "dedup" or "dense" for the test to print."""
    from dne_hip import _lib
    active, U1, U2 = engine.ref_dedup_active()
    if int(knob) != 0 and ref.shape[0] in ROUTE_FS:
        _, patches, _, windows, verdict = _lib.debug_ref_index(ref)
        assert (U1, U2) == (patches.shape[0], windows.shape[0]), ("U1 / U2 of the engine and of the host", U1, U2, patches.shape[0], windows.shape[0])
        assert bool(active) == bool(verdict), ("route of the engine and verdict of the host", active, verdict, U1, U2)
        if want_dedup is not None:
            assert bool(active) == bool(want_dedup), ("the batch was meant for the %s route" % ("dedup" if want_dedup else "dense"), U1, U2)
    else:
        assert not active and (U1, U2) == (0, 0), (knob, ref.shape[0], active, U1, U2)
    return "dedup" if active else "dense"


def fixture_frames(F=16, seed=0):
    import oracle as O
    return O.get_ref_batch(seed, F, 18, seed)


def random_frames(F=16, seed=3):
    return np.random.RandomState(seed).randint(0, 256, (F, 84, 84, 4)).astype(np.uint8)


def mixed_frames(F, k, seed=3):
    """the fixture's frames with frames 0 .. k-1 replaced by the first k of random_frames(F, seed): k = 0 is the fixture (dedup), k = F
    is all random (dense); in between the tables grow by about one frame's rows per step, up to and past what fits and pays"""
    ref = fixture_frames(F).copy()
    ref[:k] = random_frames(F, seed)[:k]
    return ref


def flat_frames(F=16, value=7):
    """F identical frames of one value: a patch differs only by how much zero padding it holds (3 x 3 kinds)"""
    return np.full((F, 84, 84, 4), value, np.uint8)


def odd_frames(F=16):
    """the fixture's frames with single pixels of frame 0 changed until U1 % 16 and U2 % 16 are both nonzero (both tables then end inside
    a tile, a step of k_conv1_ref_uniq and a step of k_conv2_ref_uniq); deterministic"""
    from dne_hip import _lib
    ref = fixture_frames(F).copy()
    for k in range(64):
        _, patches, _, windows, _ = _lib.debug_ref_index(ref)
        if patches.shape[0] % 16 and windows.shape[0] % 16:
            return ref
        ref[0, 40, (5 * k) % 84, k % 4] = 201 + k % 50
    raise AssertionError("no batch with U1 % 16 != 0 and U2 % 16 != 0 found")


# ---- csrc/ref_index.h's cost model and scratch bound, restated (constants copied by hand from the header's comment and definitions) ----
MS_CONV1_DENSE, MS_CONV2_DENSE = np.float32(18.30), np.float32(11.46)
MS_CONV1_UNIQ, MS_CONV2_UNIQ = np.float32(21.4), np.float32(16.4)
MS_GATHER = np.float32(1.71) + np.float32(3.34)
U1_PAD, U2_PAD = 32, 64                # rows per step of k_conv1_ref_uniq / k_conv2_ref_uniq
C1U_ROWS, C2U_ROWS = 32, 64            # ... the same numbers as the kernels' own row counts per step
SPW1, SPW2 = 32, 16                    # steps per workgroup segment of the two kernels (engine.hip: ref_pass)


def pad(u, to):
    return (u + to - 1) // to * to


def room(F, U1, U2):
    """floats per member left in the dense route's y1 [F][441][16] beside y1u [U1p][16] and y2u [U2p][32]; negative: they do not fit"""
    return F * N1 * 16 - (pad(U1, U1_PAD) * 16 + pad(U2, U2_PAD) * 32)


def cost(F, U1, U2):
    """the model's time of the dedup route in float32, term by term in the header's order"""
    f1 = np.float32(U1) / np.float32(F * N1)
    f2 = np.float32(U2) / np.float32(F * N2)
    return np.float32(np.float32(np.float32(MS_CONV1_UNIQ * f1) + np.float32(MS_CONV2_UNIQ * f2)) + MS_GATHER)


def pays(F, U1, U2):
    """ref_dedup_pays: cheaper than the dense kernels, and the tables fit"""
    return bool(cost(F, U1, U2) < np.float32(MS_CONV1_DENSE + MS_CONV2_DENSE)) and room(F, U1, U2) >= 0


def im2col1(ref):
    """[F][441][256] u8: the 8x8x4 patches of the zero-padded 88x88 frames at stride 4, k = (kh, kw, c)"""
    F = ref.shape[0]
    img = np.zeros((F, 88, 88, 4), np.uint8)
    img[:, 2:86, 2:86] = ref
    w = np.lib.stride_tricks.sliding_window_view(img, (8, 8), axis=(1, 2))[:, ::4, ::4]   # [F][21][21][c][kh][kw]
    return np.ascontiguousarray(w.transpose(0, 1, 2, 4, 5, 3)).reshape(F, N1, 256)


def windows2(ids1):
    """[F][121][16]: the 4x4 windows at stride 2 of the [F][441] id planes under SAME(1, 2) padding, -1 on the padding"""
    F = ids1.shape[0]
    g = np.full((F, 24, 24), -1, ids1.dtype)
    g[:, 1:22, 1:22] = ids1.reshape(F, 21, 21)
    w = np.lib.stride_tricks.sliding_window_view(g, (4, 4), axis=(1, 2))[:, ::2, ::2]      # [F][11][11][kh][kw]
    return np.ascontiguousarray(w).reshape(F, N2, 16)


def padding_mask2():
    """[121][16] bool: the taps of each conv2 position that fall on the SAME padding"""
    return windows2(np.zeros((1, N1), np.int64))[0] < 0
