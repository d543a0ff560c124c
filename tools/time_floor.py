"""Device time of one closure evaluation with the floor-contact term, beside the plain closures and the foot-lock-alone ones
(uuo_time_closure): chamfer and marker (one-hot and three-corner) stages at F x M on a capture with a floor.  The configurations
take turns inside every repeat (alternating rounds), and the medians over the repeats are printed.
python tools/time_floor.py [--frames 300 --markers 50 --points 6]"""
import argparse

import numpy as np
import torch

from closure_case import STAGES, stage_case, stage_problems, time_rounds  # (puts the repository on the path: keep it first)
from uuo_mocap_amd.body_model import sole_vertices
from uuo_mocap_amd.config import packaged_config


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--points", type=int, default=6, help="sole points K (even: K / 2 per foot)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    F, M = a.frames, a.markers
    case = stage_case(F, M, torch.device("cuda:0"), planted_feet=True, floor=True)
    contacts = case.seq.img_smpl.foot_contacts
    contact, floor = packaged_config("video_mocap_contact"), packaged_config("video_mocap_floor")
    both = packaged_config("video_mocap_floor")
    pts = [[int(v) for v in r] for r in sole_vertices(case.tables, per_foot=a.points // 2)]
    for k in ("chamfer", "marker"):
        both["stages"][k]["losses"]["foot_lock"] = contact["stages"][k]["losses"]["foot_lock"]
        for cfg in (floor, both):
            cfg["stages"][k]["floor_points"] = pts
    labels = (("plain", packaged_config("video_mocap")), ("foot_lock", contact), ("floor", floor), ("floor+foot_lock", both))
    probs = {label: stage_problems(case.smpl, case, cfg, foot_contacts=contacts) for label, cfg in labels}
    times = time_rounds([label for label, _cfg in labels], probs, case, a.repeats, a.iters)
    for label, _cfg in labels:
        line = ["%s %s us (median %.2f)" % (name, " ".join("%.1f" % v for v in times[(label, name)]), np.median(times[(label, name)]))
                for name in STAGES]
        print("closure %-16s F=%d M=%d K=%d  %s" % (label, F, M, a.points, ";  ".join(line)))


if __name__ == "__main__":
    main()
