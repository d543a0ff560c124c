"""Device time of one closure evaluation with per-(frame, joint) weights on the pose prior, beside the same build with the
weights off (uuo_time_closure): chamfer and marker (one-hot and three-corner) stages at F x M on the dropout capture's table
(gap_weight 0, ramp 0), alone and on top of the joint-acceleration term (whose kernels are the temporal family the weights
select, so that pair isolates k_prior_conf itself).  The configurations take turns inside every repeat (alternating rounds),
and the medians over the repeats are printed.
python tools/time_prior_confidence.py [--frames 300 --markers 50]"""
import argparse

import numpy as np
import torch

from closure_case import STAGES, stage_case, stage_problems, time_rounds  # (puts the repository on the path: keep it first)
from uuo_mocap_amd.config import packaged_config
from uuo_mocap_amd.engine import prior_weight_table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    F, M = a.frames, a.markers
    case = stage_case(F, M, torch.device("cuda:0"), video_dropout=True)
    w = prior_weight_table(case.seq.img_smpl.img_mask, {"gap_weight": 0.0, "ramp": 0, "joint_weights": None})
    plain, accel = packaged_config("video_mocap"), packaged_config("video_mocap_smooth")
    labels = (("plain", plain, None), ("weights", plain, w), ("joint_accel", accel, None), ("joint_accel+weights", accel, w))
    probs = {label: stage_problems(case.smpl, case, cfg, prior_weights=tab) for label, cfg, tab in labels}
    times = time_rounds([label for label, _cfg, _tab in labels], probs, case, a.repeats, a.iters)
    for label, _cfg, _tab in labels:
        line = ["%s %s us (median %.2f)" % (name, " ".join("%.1f" % v for v in times[(label, name)]), np.median(times[(label, name)]))
                for name in STAGES]
        print("closure %-20s F=%d M=%d  %s" % (label, F, M, ";  ".join(line)))


if __name__ == "__main__":
    main()
