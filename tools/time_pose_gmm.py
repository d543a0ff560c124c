"""Device time of one closure evaluation with the mixture pose prior, beside the plain closures, the joint_accel-alone ones and
the joint-angle limit term (uuo_time_closure): chamfer and marker (one-hot and three-corner) stages at F x M with the stand-in
mixture at K components, and one more row at --more components.  The configurations take turns inside every repeat
(alternating rounds), and the medians over the repeats are printed with each configuration's increment over joint_accel alone
(the temporal kernels: what any side term of this kind runs on).
python tools/time_pose_gmm.py [--frames 300 --markers 50 --components 8 --more 16]"""
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
from uuo_mocap_amd.synthetic import make_sequence, pose_mixture  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--components", type=int, default=8)
    ap.add_argument("--more", type=int, default=16, help="components of the extra row (0 = none)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tables = synthetic_smpl(0)
    smpl = SmplInference(dev, tables=tables)
    F, M = a.frames, a.markers
    seq = make_sequence(tables, seed=0, num_frames=F, num_markers=M)
    markers = torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float().to(dev)
    o_pose = seq.img_smpl.pose_body.float().to(dev)
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).float().to(dev)
    root = seq.img_smpl.root_orient.float().to(dev)
    trans = torch.median(markers, dim=1)[0]
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32).to(dev)
    faces = torch.from_numpy(np.asarray(tables.faces).astype(np.int64))
    i3 = torch.stack([torch.sort(faces[(faces == int(v)).any(1).nonzero()[0, 0]])[0] for v in vids.cpu()]).to(torch.int32).to(dev)
    b3 = torch.full((M, 3), 1.0 / 3.0, device=dev)
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
    probs, times = {}, {}
    for label, cfg, mix in labels:
        kw = {} if mix is None else {"pose_mixture": mix}
        probs[label] = {
            "chamfer": ChamferProblem(smpl, markers, o_pose, o_betas, root, cfg, **kw),
            "marker": MarkerProblem(smpl, markers, o_pose, o_betas, vids, cfg, **kw),
            "marker3": MarkerProblem(smpl, markers, o_pose, o_betas, i3, cfg, bary=b3, **kw),
        }
    for _ in range(a.repeats):  # alternating rounds: every configuration once per repeat
        for label, _cfg, _mix in labels:
            for name, p in probs[label].items():
                x = p.pack(trans, torch.zeros(F, 1, 1, device=dev), o_betas, o_pose) if name == "chamfer" else \
                    p.pack(o_pose, o_betas, root, trans)
                times.setdefault((label, name), []).append(p.time_closure(x, iters=a.iters) * 1e3)
    med = {key: float(np.median(v)) for key, v in times.items()}
    for label, _cfg, _mix in labels:
        line = ["%s %s us (median %.2f, %+.2f over joint_accel)"
                % (name, " ".join("%.1f" % v for v in times[(label, name)]), med[(label, name)], med[(label, name)] - med[("joint_accel", name)])
                for name in ("chamfer", "marker", "marker3")]
        print("closure %-28s F=%d M=%d  %s" % (label, F, M, ";  ".join(line)))


if __name__ == "__main__":
    main()
