"""Device time of one closure evaluation with the fused pose-acceleration term (k_pose_accel), beside the
plain closures and -- the yardstick, in the same call -- the joint-angle limit term's (k_limit_fwd, the kernel whose shape it
has): chamfer and marker (one-hot and three-corner) stages at F x M (uuo_time_closure).  The configurations take turns inside
every repeat (alternating rounds), and the medians over the repeats are printed with each term's increment over the plain
closure.  With --fit, one full fit of the capture with video_mocap_rotsmooth_fused.yaml follows (wall time after a warm-up fit
of video_mocap.yaml), and with --composed the same fit with video_mocap_rotsmooth.yaml, the term on the composed closures.
python tools/time_pose_accel.py [--frames 300 --markers 50] [--fit] [--composed]"""
import argparse
import copy
import time

import numpy as np
import torch

from closure_case import STAGES, stage_case, stage_problems, time_rounds  # (puts the repository on the path: keep it first)
from uuo_mocap_amd.config import packaged_config
from uuo_mocap_amd.synthetic import SyntheticMarkers


def _fit(seq, name, smpl, dev):
    from uuo_mocap_amd.multimodal import multimodal_video_mocap

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(np.asarray(seq.markers.get_points()).copy(), 30.0), dev,
                           packaged_config(name), offset=0, print_options=[], save_stages=False, smpl_inference=smpl)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--composed", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    F, M = a.frames, a.markers
    case = stage_case(F, M, dev)
    seq, smpl = case.seq, case.smpl
    fused = packaged_config("video_mocap_rotsmooth_fused")
    both = packaged_config("video_mocap_limits")
    both["execution"] = dict(both.get("execution") or {}, pose_accel_fused=True)
    for k in ("chamfer", "marker"):
        both["stages"][k]["losses"]["pose_accel"] = fused["stages"][k]["losses"]["pose_accel"]
    labels = (("plain", packaged_config("video_mocap")), ("joint_limits", packaged_config("video_mocap_limits")),
              ("pose_accel", fused), ("pose_accel+joint_limits", both))
    probs = {}
    for label, cfg in labels:
        probs[label] = stage_problems(smpl, case, cfg)
        assert all(p.pose_accel_on == label.startswith("pose_accel") for p in probs[label].values())
    times = time_rounds([label for label, _cfg in labels], probs, case, a.repeats, a.iters)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for label, _cfg in labels:
        line = ["%s %s us (median %.2f, %+.2f over plain)" % (name, " ".join("%.1f" % v for v in times[(label, name)]),
                                                              med[(label, name)], med[(label, name)] - med[("plain", name)])
                for name in STAGES]
        print("closure %-24s F=%d M=%d  %s" % (label, F, M, ";  ".join(line)))
    if a.fit or a.composed:
        _fit(seq, "video_mocap", smpl, dev)  # warm-up: workspaces, the first launches
        names = ["video_mocap"] + (["video_mocap_rotsmooth_fused"] if a.fit else []) + (["video_mocap_rotsmooth"] if a.composed else [])
        for name in names:
            print("fit %-30s F=%d M=%d  %.2f s" % (name, F, M, _fit(seq, name, smpl, dev)), flush=True)


if __name__ == "__main__":
    main()
