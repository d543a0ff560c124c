"""Device time of one closure evaluation with the mixture pose prior, beside the plain closures, the joint_accel-alone ones and
the joint-angle limit term (uuo_time_closure): chamfer and marker (one-hot and three-corner) stages at F x M with the stand-in
mixture at K components, and one more row at --more components.  The configurations take turns inside every repeat
(alternating rounds), and the medians over the repeats are printed with each configuration's increment over joint_accel alone
(the temporal kernels: what any side term of this kind runs on).
python tools/time_pose_gmm.py [--frames 300 --markers 50 --components 8 --more 16]"""
import argparse

import numpy as np
import torch

from closure_case import STAGES, stage_case, stage_problems, time_rounds  # (puts the repository on the path: keep it first)
from uuo_mocap_amd.config import packaged_config
from uuo_mocap_amd.synthetic import pose_mixture


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--components", type=int, default=8)
    ap.add_argument("--more", type=int, default=16, help="components of the extra row (0 = none)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    F, M = a.frames, a.markers
    case = stage_case(F, M, torch.device("cuda:0"))
    lim = packaged_config("video_mocap_limits")

    def gmm_cfg(limits):
        cfg = packaged_config("video_mocap_limits" if limits else "video_mocap")
        for k, w in (("chamfer", 0.01), ("marker", 0.001)):
            cfg["stages"][k]["losses"]["pose_gmm"] = w
        return cfg

    labels = [("plain", packaged_config("video_mocap"), None), ("joint_accel", packaged_config("video_mocap_smooth"), None),
              ("joint_limits", lim, None), ("pose_gmm K=%d" % a.components, gmm_cfg(False), pose_mixture(K=a.components)),
              ("pose_gmm K=%d+joint_limits" % a.components, gmm_cfg(True), pose_mixture(K=a.components))]
    if a.more:
        labels.append(("pose_gmm K=%d" % a.more, gmm_cfg(False), pose_mixture(K=a.more)))
    probs = {label: stage_problems(case.smpl, case, cfg, **({} if mix is None else {"pose_mixture": mix})) for label, cfg, mix in labels}
    times = time_rounds([label for label, _cfg, _mix in labels], probs, case, a.repeats, a.iters)
    med = {key: float(np.median(v)) for key, v in times.items()}
    for label, _cfg, _mix in labels:
        line = ["%s %s us (median %.2f, %+.2f over joint_accel)"
                % (name, " ".join("%.1f" % v for v in times[(label, name)]), med[(label, name)], med[(label, name)] - med[("joint_accel", name)])
                for name in STAGES]
        print("closure %-28s F=%d M=%d  %s" % (label, F, M, ";  ".join(line)))


if __name__ == "__main__":
    main()
