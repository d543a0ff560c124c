"""Device time of one closure evaluation with the bone-capsule self-penetration term, beside the plain closures and the
joint_accel-alone ones (uuo_time_closure): chamfer and marker (one-hot and three-corner) stages at F x M with the builder's
capsule list.  The configurations take turns inside every repeat (alternating rounds), and the medians over the repeats are
printed.
python tools/time_capsules.py [--frames 300 --markers 50 --pairs 232]"""
import argparse

import numpy as np
import torch

from closure_case import STAGES, stage_case, stage_problems, time_rounds  # (puts the repository on the path: keep it first)
from uuo_mocap_amd.body_model import body_capsules
from uuo_mocap_amd.config import packaged_config


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=0, help="use the first N pairs of the builder's list (0: all)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    F, M = a.frames, a.markers
    case = stage_case(F, M, torch.device("cuda:0"))
    cj, cg, pr = body_capsules(case.tables)
    if a.pairs:
        pr = pr[:a.pairs]
    block = {"joints": cj.tolist(), "geom": [[float(v) for v in r] for r in cg], "pairs": pr.tolist()}
    accel, caps, both = (packaged_config(n) for n in ("video_mocap_smooth", "video_mocap_capsules", "video_mocap_smooth"))
    for k in ("chamfer", "marker"):
        both["stages"][k]["losses"]["self_penetration"] = caps["stages"][k]["losses"]["self_penetration"]
        for cfg in (caps, both):
            cfg["stages"][k]["capsules"] = block
    labels = (("plain", packaged_config("video_mocap")), ("joint_accel", accel), ("capsules", caps), ("capsules+joint_accel", both))
    probs = {label: stage_problems(case.smpl, case, cfg) for label, cfg in labels}
    times = time_rounds([label for label, _cfg in labels], probs, case, a.repeats, a.iters)
    for label, _cfg in labels:
        line = ["%s %s us (median %.2f)" % (name, " ".join("%.1f" % v for v in times[(label, name)]), np.median(times[(label, name)]))
                for name in STAGES]
        print("closure %-21s F=%d M=%d P=%d  %s" % (label, F, M, len(pr), ";  ".join(line)))


if __name__ == "__main__":
    main()
