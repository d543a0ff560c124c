"""Device time of one closure evaluation with the 2D key-point reprojection term, beside the plain closures
and -- the yardstick, in the same call -- the joint-angle limit term's (k_limit_fwd, a kernel of the same shape): chamfer and
marker (one-hot and three-corner) stages at F x M (uuo_time_closure).  The evidence is synthetic_keypoints_2d of the capture.  The
configurations take turns inside every repeat (alternating rounds), and the medians over the repeats are printed with each
term's increment over the plain closure.
python tools/time_keypoints2d.py [--frames 300 --markers 50]"""
import argparse

import numpy as np
import torch

from closure_case import STAGES, stage_case, stage_problems, time_rounds  # (puts the repository on the path: keep it first)
from uuo_mocap_amd.config import packaged_config
from uuo_mocap_amd.synthetic import synthetic_keypoints_2d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--weight", type=float, default=1e-3)
    ap.add_argument("--sigma", type=float, default=20.0)
    a = ap.parse_args()
    F, M = a.frames, a.markers
    case = stage_case(F, M, torch.device("cuda:0"))
    rec = synthetic_keypoints_2d(case.seq)
    keyed, both = packaged_config("video_mocap"), packaged_config("video_mocap_limits")
    for cfg in (keyed, both):
        for k in ("chamfer", "marker"):
            cfg["stages"][k]["losses"]["keypoints_2d"] = a.weight
            cfg["stages"][k]["keypoints_2d"] = {"sigma": a.sigma, "min_depth": 0.1, "joint_weights": None}
    labels = (("plain", packaged_config("video_mocap"), None), ("joint_limits", packaged_config("video_mocap_limits"), None),
              ("keypoints_2d", keyed, rec), ("keypoints_2d+joint_limits", both, rec))
    probs = {}
    for label, cfg, r in labels:
        probs[label] = stage_problems(case.smpl, case, cfg, keypoints_2d=r)
        assert all(p.keypoints_on == (r is not None) for p in probs[label].values())
    times = time_rounds([label for label, _cfg, _r in labels], probs, case, a.repeats, a.iters)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for label, _cfg, _r in labels:
        line = ["%s %s us (median %.2f, %+.2f over plain)" % (name, " ".join("%.1f" % v for v in times[(label, name)]),
                                                              med[(label, name)], med[(label, name)] - med[("plain", name)])
                for name in STAGES]
        print("closure %-26s F=%d M=%d  %s" % (label, F, M, ";  ".join(line)))


if __name__ == "__main__":
    main()
