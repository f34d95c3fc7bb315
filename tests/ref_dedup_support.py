"""TEST-ONLY: the reference batches of the unique-operand reference pass (csrc/ref_index.h) and the numpy side of its index:
tests/test_ref_index_cpu.py (the index against numpy) and tests/test_gpu_ref_dedup.py (the pass against the oracle, bit for bit)."""
import numpy as np

N1, N2 = 441, 121


def fixture_frames(F=16, seed=0):
    import oracle as O
    return O.get_ref_batch(seed, F, 18, seed)


def random_frames(F=16, seed=3):
    return np.random.RandomState(seed).randint(0, 256, (F, 84, 84, 4)).astype(np.uint8)


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
