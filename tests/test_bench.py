"""bench.py's host side (CPU): what a plain run does and the threaded generation of its synthetic inputs."""
import sys

import numpy as np
import torch

import bench
from uuo_mocap_amd.synthetic import make_sequence


def _same_sequence(a, b):
    for f in ("trans", "root_orient", "hmr_root_orient", "pose_body", "betas", "img_mask"):
        assert torch.equal(getattr(a.img_smpl, f), getattr(b.img_smpl, f)), f
    assert np.array_equal(a.markers.get_points(), b.markers.get_points())
    assert a.gt.keys() == b.gt.keys()
    for k in a.gt:
        assert np.array_equal(a.gt[k], b.gt[k]), k


def test_host_map_builds_the_same_sequences_in_order(tables):
    # the timed steps' inputs must not depend on how they were generated
    def gen(i):
        return make_sequence(tables, seed=i, num_frames=24, num_markers=10 if i == 3 else 50, limb_only=i == 3,
                             subject_seed=5000 + i if i == 2 else None)

    threaded = bench.host_map(gen, range(5))
    assert len(threaded) == 5
    for i, s in enumerate(threaded):
        _same_sequence(s, gen(i))


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1"])
    assert not bench.parse().full
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full
