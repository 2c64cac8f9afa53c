"""Cases shared by tests/test_voxel_cpu.py and tests/test_hip_voxel.py: the hand-made rows of the voxel rule with the
answers worked out by hand, a seeded cloud, and the descriptors that gs_voxel_keep_dc_f32 must refuse before any HIP
call.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

f32 = np.float32
NAN, INF = float("nan"), float("inf")
VS = 0.0625                      # a voxel size that float32 holds exactly
BELOW = float(np.nextafter(f32(65536.0), f32(0)))        # the largest float below 2^20 voxels: q = 2^20 - 1
BEYOND = float(np.nextafter(f32(-65536.0), f32(-INF)))   # the first float below -2^20 voxels: q = -2^20 - 1

# (point, confidence, winner of the row's voxel with the confidences, winner without them, what the row is there for)
ROWS = [
    ((0.1875, 0.0, 0.0), 1.0, 1, 0, "exactly on a voxel face: 3 * 0.0625 belongs to voxel 3"),
    ((0.1975, 0.01, 0.01), 2.0, 1, 0, "the same voxel, more confident"),
    ((float(np.nextafter(f32(0.1875), f32(0))), 0.0, 0.0), 0.5, 2, 2, "one ulp below the face: voxel 2, alone"),
    ((-0.03, 0.0, 0.0), 1.0, 3, 3, "a negative coordinate: voxel -1, not 0"),
    ((-0.0625, 0.0, 0.0), 1.0, 3, 3, "on the face of voxel -1; a confidence tie: the lower row wins"),
    ((-0.0, -0.0, -0.0), 0.25, 5, 5, "-0.0 is voxel 0"),
    ((0.0, 0.03, 0.03), 0.25, 5, 5, "voxel 0 with +0.0, a tie"),
    ((65536.0, 0.0, 0.0), 9.0, 7, 7, "q = 2^20: not griddable, kept"),
    ((BELOW, 0.0, 0.0), 1.0, 8, 8, "the largest float below it: q = 2^20 - 1, griddable, alone"),
    ((65536.0, 0.0, 0.0), 1.0, 9, 9, "identical to row 7 and out of range: both kept, no competition"),
    ((-65536.0, 0.0, 0.0), 1.0, 10, 10, "q = -2^20: the lower limit is inside"),
    ((BEYOND, 0.0, 0.0), 1.0, 11, 11, "q = -2^20 - 1: not griddable"),
    ((NAN, 0.0, 0.0), 1.0, 12, 12, "NaN coordinate"),
    ((0.0, INF, 0.0), 1.0, 13, 13, "+inf coordinate"),
    ((0.0, 0.0, -INF), 1.0, 14, 14, "-inf coordinate"),
    ((1.0, 1.0, 1.0), NAN, 15, 15, "NaN confidence scores 0"),
    ((1.0, 1.0, 1.0), -5.0, 15, 15, "negative confidence scores 0: a tie with the NaN"),
    ((1.01, 1.01, 1.01), -0.0, 15, 15, "-0.0 scores as +0.0: a tie"),
    ((2.0, 2.0, 2.0), 3.0, 19, 18, "an ordinary confidence"),
    ((2.0, 2.0, 2.0), INF, 19, 18, "+inf is the largest"),
    ((2.01, 2.0, 2.0), 1e30, 19, 18, "large, but finite"),
    ((3.0, 3.0, 3.0), NAN, 22, 21, "NaN loses to anything positive"),
    ((3.0, 3.0, 3.0), 1e-45, 22, 21, "the smallest denormal: bit pattern 1"),
    ((4.0, 4.0, 4.0), -0.0, 23, 23, "-0.0 against +0.0 is a tie: the lower row"),
    ((4.0, 4.0, 4.0), 0.0, 23, 23, "+0.0"),
    ((5.0, 0.0, 0.0), 1.0, 25, 25, "differs from the next row in y only"),
    ((5.0, 0.07, 0.0), 2.0, 26, 26, "... another voxel"),
    ((5.0, 0.0, 0.07), 2.0, 27, 27, "differs from row 25 in z only"),
]
POINTS = np.array([r[0] for r in ROWS], f32)
CONF = np.array([r[1] for r in ROWS], f32)
WINNER = np.array([r[2] for r in ROWS], np.int64)
WINNER_PLAIN = np.array([r[3] for r in ROWS], np.int64)
GRIDDABLE = np.array([i not in (7, 9, 11, 12, 13, 14) for i in range(len(ROWS))])


def cloud(n=5000, seed=7, side=1.0):
    """(points (n, 3), confidence (n,)): a seeded cloud in a cube of `side` metres with confidences that tie often, and a
    sprinkle of rows that cannot be put on the grid"""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-side / 2, side / 2, (n, 3)).astype(f32)
    C = rng.integers(0, 6, n).astype(f32) * f32(0.5)
    bad = rng.choice(n, max(n // 100, 1), replace=False)
    P[bad[::3], 0] = NAN
    P[bad[1::3], 1] = INF
    P[bad[2::3], 2] = 1e9
    C[rng.choice(n, max(n // 50, 1), replace=False)] = NAN
    return P, C


# ------------------------------------------------------------------------------------------ the C entry point
def seq(**kw):
    """a descriptor that passes every check (fake non-NULL pointers: nothing is dereferenced before a HIP call, and every
    case below is rejected before one)"""
    d = dict(points=0x1000, confidence=0x2000, n_bound=100, n_dev=0, keep=0x3000, winner=0x4000, unplaced=0x5000,
             scratch=0x10000, scratch_bytes=1 << 20)
    d.update(kw)
    return d


INVALID = {
    "null_points": (dict(points=0), {}, "NULL"),
    "null_both_outputs": (dict(keep=0, winner=0), {}, "NULL"),
    "null_scratch": (dict(scratch=0), {}, "NULL"),
    "small_scratch": (dict(scratch_bytes=1024 * 16 - 1), {}, "scratch"),
    "small_scratch_for_the_bound": (dict(n_bound=513, scratch_bytes=2048 * 16 - 1), {}, "scratch"),
    "misaligned_scratch": (dict(scratch=0x10008), {}, "aligned"),
    "misaligned_winner": (dict(winner=0x4004), {}, "aligned"),
    "negative_bound": (dict(n_bound=-1), {}, "n_bound"),
    "too_many_rows": (dict(n_bound=1 << 31, scratch_bytes=1 << 62), {}, "n_bound"),
    "no_sequences": ({}, dict(B=0), "bad arguments"),
    "negative_batch": ({}, dict(B=-2), "bad arguments"),
    "zero_voxel": ({}, dict(voxel_size=0.0), "voxel_size"),
    "negative_voxel": ({}, dict(voxel_size=-0.01), "voxel_size"),
    "nan_voxel": ({}, dict(voxel_size=NAN), "voxel_size"),
    "infinite_voxel": ({}, dict(voxel_size=INF), "voxel_size"),
}


def fill(q, d):
    for k, v in d.items():
        setattr(q, k, v)


def check_refusal(_C, case):
    lib = _C.lib()
    change, args, word = INVALID[case]
    seqs = (_C.VoxelKeepSeq * 1)()
    fill(seqs[0], seq(**change))
    a = dict(dict(B=1, voxel_size=VS), **args)
    assert lib.gs_voxel_keep_dc_f32(seqs, a["B"], a["voxel_size"], None) == 1       # GS_ERR_INVALID
    assert word in lib.gs_last_error().decode(), lib.gs_last_error()


def check_refusals_of_the_batch(_C):
    """every sequence is checked, and the descriptor pointer itself"""
    lib = _C.lib()
    seqs = (_C.VoxelKeepSeq * 2)()
    for q in seqs:
        fill(q, seq())
    assert lib.gs_voxel_keep_dc_f32(None, 1, VS, None) == 1
    fill(seqs[1], seq(points=0))
    assert lib.gs_voxel_keep_dc_f32(seqs, 2, VS, None) == 1
    assert "NULL" in lib.gs_last_error().decode()
    # the table: the power of two >= max(2 n_bound, 1024) slots of 16 bytes, 32 - 64 bytes per row of the bound
    size = lib.gs_voxel_keep_scratch_bytes
    assert [size(n) for n in (-5, 0, 1, 512, 513, 1024, 1025, 1 << 20)] == \
        [16 * c for c in (1024, 1024, 1024, 1024, 2048, 2048, 4096, 1 << 21)]
    for n in (600, 1000, 4097, 2_600_000, 10_000_000):
        assert 32 * n <= size(n) < 64 * n
