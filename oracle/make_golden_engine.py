"""The ORACLE (oracle/slam.py: the C restatement, oracle/gs_oracle.c) on the scenes of the ICP engine matrix
(tests/test_hip_engine_matrix.py): every engine switch of the HIP solve must reproduce these poses bit for bit.

    python -m oracle.make_golden_engine                 # all four scenes
    python -m oracle.make_golden_engine --scene hard3

Scenes (PointFusion, gradICP, defaults; poses[1:] = poses[:1] as tests/test_hip_batch.py::_LIST_SCRIPT does; sequence b
is make_sequence(L, H, W, seed=seeds[b], first=first)):
    bench8   8 x 480x640, frames 0..3     the benchmark's shard, where the persistent solve was measured
    hard3    3 x 480x640, frames 85..88   cube scans, wide lists, block-wide passes (grazing frame border)
    ragged2  2 x 67x131, frames 0..3      561-point lattice: the last row unit of 96 points is partial
    weak1    1 x 480x640, frames 0..8     frame 8: ~5 % of the points get weak lists (GRADSLAM_HIP_ICP_WEAK_ROOM)

Build-container only (a few CPU minutes).  Output: tests/golden/engine_<scene>_oracle.npz with per sequence the depth
checksum, poses (L,4,4) f32, counts (L,), float64 point sums per frame and a seeded sample of SAMPLE rows of the final
map (row indices + points).  TEST INFRASTRUCTURE ONLY."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from gradslam_amd.datasets.synthetic import make_sequence  # noqa: E402
from oracle import slam as oslam  # noqa: E402

SCENES = {
    "bench8": dict(H=480, W=640, L=4, first=0, seeds=list(range(3, 11))),
    "hard3": dict(H=480, W=640, L=4, first=85, seeds=[3, 4, 5]),
    "ragged2": dict(H=67, W=131, L=4, first=0, seeds=[3, 4]),
    "weak1": dict(H=480, W=640, L=9, first=0, seeds=[0]),
}
SAMPLE = 4096         # map rows kept per sequence
SAMPLE_SEED = 20261016


def golden_path(scene):
    return os.path.join(REPO, "tests", "golden", "engine_%s_oracle.npz" % scene)


def sequence_inputs(scene, b):
    c = SCENES[scene]
    return make_sequence(c["L"], c["H"], c["W"], seed=c["seeds"][b], first=c["first"])


def run_one(scene, b, log=None):
    """The oracle's record of sequence b of `scene` (what one row of the fixture holds)."""
    s = sequence_inputs(scene, b)
    poses = s["poses"].copy()
    poses[1:] = poses[:1]
    counts, sums = [], []
    t0 = time.time()

    def rec(f, m, p):
        counts.append(len(m))
        sums.append(m.points.astype(np.float64).sum(0))
        if log:
            log("%s[%d] frame %d  %d surfels  %.1f s" % (scene, b, f, len(m), time.time() - t0))

    m, rp = oslam.run_sequence(s["colors"], s["depths"], s["intrinsics"][0], poses, per_frame=rec)
    n = len(m)
    assert n >= SAMPLE, (scene, b, n)
    idx = np.sort(np.random.default_rng([SAMPLE_SEED, b]).choice(n, size=SAMPLE, replace=False)).astype(np.int32)
    return dict(depth_sum=float(s["depths"].astype(np.float64).sum()), poses=rp.astype(np.float32),
                counts=np.asarray(counts, np.int64), sum_points=np.asarray(sums, np.float64), sample_idx=idx,
                sample_points=np.ascontiguousarray(m.points[idx], np.float32))


def make(scene, log=print):
    c = SCENES[scene]
    rows = [run_one(scene, b, log) for b in range(len(c["seeds"]))]
    out = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    np.savez_compressed(golden_path(scene), H=np.int64(c["H"]), W=np.int64(c["W"]), L=np.int64(c["L"]),
                        first=np.int64(c["first"]), seeds=np.asarray(c["seeds"], np.int64), **out)
    return golden_path(scene)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=sorted(SCENES), action="append")
    a = ap.parse_args()
    for scene in a.scene or list(SCENES):
        p = make(scene)
        print("wrote %s (%d bytes)" % (p, os.path.getsize(p)), flush=True)


if __name__ == "__main__":
    main()
