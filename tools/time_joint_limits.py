"""Device time of one closure evaluation with the joint-angle limit term, beside the plain closures and the joint_accel-alone
ones (uuo_time_closure): chamfer and marker (one-hot and three-corner) stages at F x M with the builder's table, or with every
component bounded (--full: the kernel's work does not depend on the table, only its hinges do).  The configurations take turns
inside every repeat (alternating rounds), and the medians over the repeats are printed.
python tools/time_joint_limits.py [--frames 300 --markers 50 --full]"""
import argparse

import numpy as np
import torch

from closure_case import STAGES, stage_case, stage_problems, time_rounds  # (puts the repository on the path: keep it first)
from uuo_mocap_amd.config import packaged_config


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--full", action="store_true", help="bound every component at +-0.2 rad instead of the builder's table")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    F, M = a.frames, a.markers
    case = stage_case(F, M, torch.device("cuda:0"))
    block = {"lo": [[-0.2] * 3] * 23, "hi": [[0.2] * 3] * 23} if a.full else None
    accel, lim, both = (packaged_config(n) for n in ("video_mocap_smooth", "video_mocap_limits", "video_mocap_smooth"))
    for k in ("chamfer", "marker"):
        both["stages"][k]["losses"]["joint_limits"] = lim["stages"][k]["losses"]["joint_limits"]
        for cfg in (lim, both):
            cfg["stages"][k]["joint_limits"] = block
    labels = (("plain", packaged_config("video_mocap")), ("joint_accel", accel), ("joint_limits", lim), ("joint_limits+joint_accel", both))
    probs = {label: stage_problems(case.smpl, case, cfg) for label, cfg in labels}
    times = time_rounds([label for label, _cfg in labels], probs, case, a.repeats, a.iters)
    for label, _cfg in labels:
        line = ["%s %s us (median %.2f)" % (name, " ".join("%.1f" % v for v in times[(label, name)]), np.median(times[(label, name)]))
                for name in STAGES]
        print("closure %-25s F=%d M=%d table=%s  %s" % (label, F, M, "full" if a.full else "builder", ";  ".join(line)))


if __name__ == "__main__":
    main()
