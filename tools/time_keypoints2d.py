"""Device time of one closure evaluation with the 2D key-point reprojection term, beside the plain closures
and -- the yardstick, in the same call -- the joint-angle limit term's (k_limit_fwd, a kernel of the same shape): chamfer and
marker (one-hot and three-corner) stages at F x M (uuo_time_closure).  The evidence is synthetic_keypoints_2d of the capture.  The
configurations take turns inside every repeat (alternating rounds), and the medians over the repeats are printed with each
term's increment over the plain closure.
python tools/time_keypoints2d.py [--frames 300 --markers 50]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uuo_mocap_amd.body_model import synthetic_smpl  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence, synthetic_keypoints_2d  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--weight", type=float, default=1e-3)
    ap.add_argument("--sigma", type=float, default=20.0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tables = synthetic_smpl(0)
    smpl = SmplInference(dev, tables=tables)
    F, M = a.frames, a.markers
    seq = make_sequence(tables, seed=0, num_frames=F, num_markers=M)
    rec = synthetic_keypoints_2d(seq)
    markers = torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float().to(dev)
    o_pose = seq.img_smpl.pose_body.float().to(dev)
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).float().to(dev)
    root = seq.img_smpl.root_orient.float().to(dev)
    trans = torch.median(markers, dim=1)[0]
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32).to(dev)
    faces = torch.from_numpy(np.asarray(tables.faces).astype(np.int64))
    i3 = torch.stack([torch.sort(faces[(faces == int(v)).any(1).nonzero()[0, 0]])[0] for v in vids.cpu()]).to(torch.int32).to(dev)
    b3 = torch.full((M, 3), 1.0 / 3.0, device=dev)
    keyed, both = packaged_config("video_mocap"), packaged_config("video_mocap_limits")
    for cfg in (keyed, both):
        for k in ("chamfer", "marker"):
            cfg["stages"][k]["losses"]["keypoints_2d"] = a.weight
            cfg["stages"][k]["keypoints_2d"] = {"sigma": a.sigma, "min_depth": 0.1, "joint_weights": None}
    labels = (("plain", packaged_config("video_mocap"), None), ("joint_limits", packaged_config("video_mocap_limits"), None),
              ("keypoints_2d", keyed, rec), ("keypoints_2d+joint_limits", both, rec))
    probs, times = {}, {}
    for label, cfg, r in labels:
        probs[label] = {
            "chamfer": ChamferProblem(smpl, markers, o_pose, o_betas, root, cfg, keypoints_2d=r),
            "marker": MarkerProblem(smpl, markers, o_pose, o_betas, vids, cfg, keypoints_2d=r),
            "marker3": MarkerProblem(smpl, markers, o_pose, o_betas, i3, cfg, bary=b3, keypoints_2d=r),
        }
        assert all(p.keypoints_on == (r is not None) for p in probs[label].values())
    for _ in range(a.repeats):  # alternating rounds: every configuration once per repeat
        for label, _cfg, _r in labels:
            for name, p in probs[label].items():
                x = p.pack(trans, torch.zeros(F, 1, 1, device=dev), o_betas, o_pose) if name == "chamfer" else \
                    p.pack(o_pose, o_betas, root, trans)
                times.setdefault((label, name), []).append(p.time_closure(x, iters=a.iters) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for label, _cfg, _r in labels:
        line = ["%s %s us (median %.2f, %+.2f over plain)" % (name, " ".join("%.1f" % v for v in times[(label, name)]),
                                                              med[(label, name)], med[(label, name)] - med[("plain", name)])
                for name in ("chamfer", "marker", "marker3")]
        print("closure %-26s F=%d M=%d  %s" % (label, F, M, ";  ".join(line)))


if __name__ == "__main__":
    main()
