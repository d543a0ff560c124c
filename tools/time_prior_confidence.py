"""Device time of one closure evaluation with per-(frame, joint) weights on the pose prior, beside the same build with the
weights off (uuo_time_closure): chamfer and marker (one-hot and three-corner) stages at F x M on the dropout capture's table
(gap_weight 0, ramp 0), alone and on top of the joint-acceleration term (whose kernels are the temporal family the weights
select, so that pair isolates k_prior_conf itself).  The configurations take turns inside every repeat (alternating rounds),
and the medians over the repeats are printed.
python tools/time_prior_confidence.py [--frames 300 --markers 50]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uuo_mocap_amd.body_model import synthetic_smpl  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem, prior_weight_table  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tables = synthetic_smpl(0)
    smpl = SmplInference(dev, tables=tables)
    F, M = a.frames, a.markers
    seq = make_sequence(tables, seed=0, num_frames=F, num_markers=M, video_dropout=True)
    markers = torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float().to(dev)
    o_pose = seq.img_smpl.pose_body.float().to(dev)
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).float().to(dev)
    root = seq.img_smpl.root_orient.float().to(dev)
    trans = torch.median(markers, dim=1)[0]
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32).to(dev)
    faces = torch.from_numpy(np.asarray(tables.faces).astype(np.int64))
    i3 = torch.stack([torch.sort(faces[(faces == int(v)).any(1).nonzero()[0, 0]])[0] for v in vids.cpu()]).to(torch.int32).to(dev)
    b3 = torch.full((M, 3), 1.0 / 3.0, device=dev)
    w = prior_weight_table(seq.img_smpl.img_mask, {"gap_weight": 0.0, "ramp": 0, "joint_weights": None})
    plain, accel = packaged_config("video_mocap"), packaged_config("video_mocap_smooth")
    labels = (("plain", plain, None), ("weights", plain, w), ("joint_accel", accel, None), ("joint_accel+weights", accel, w))
    probs, times = {}, {}
    for label, cfg, tab in labels:
        probs[label] = {
            "chamfer": ChamferProblem(smpl, markers, o_pose, o_betas, root, cfg, prior_weights=tab),
            "marker": MarkerProblem(smpl, markers, o_pose, o_betas, vids, cfg, prior_weights=tab),
            "marker3": MarkerProblem(smpl, markers, o_pose, o_betas, i3, cfg, bary=b3, prior_weights=tab),
        }
    for _ in range(a.repeats):  # alternating rounds: every configuration once per repeat
        for label, _cfg, _tab in labels:
            for name, p in probs[label].items():
                x = p.pack(trans, torch.zeros(F, 1, 1, device=dev), o_betas, o_pose) if name == "chamfer" else \
                    p.pack(o_pose, o_betas, root, trans)
                times.setdefault((label, name), []).append(p.time_closure(x, iters=a.iters) * 1e3)
    for label, _cfg, _tab in labels:
        line = ["%s %s us (median %.2f)" % (name, " ".join("%.1f" % v for v in times[(label, name)]), np.median(times[(label, name)]))
                for name in ("chamfer", "marker", "marker3")]
        print("closure %-20s F=%d M=%d  %s" % (label, F, M, ";  ".join(line)))


if __name__ == "__main__":
    main()
