"""Device time of one marker-stage closure evaluation with the latent marker offsets off and on (uuo_time_closure), one-hot
and three-corner placements at F x M.  python tools/time_marker_offsets.py [--frames 300 --markers 50]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uuo_mocap_amd.body_model import synthetic_smpl  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.engine import MarkerProblem  # noqa: E402
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
    for label, cfg in (("off", packaged_config("video_mocap")), ("on", packaged_config("video_mocap_offsets"))):
        line = []
        for name, p in (("marker", MarkerProblem(smpl, markers, o_pose, o_betas, vids, cfg)),
                        ("marker3", MarkerProblem(smpl, markers, o_pose, o_betas, i3, cfg, bary=b3))):
            x = p.pack(o_pose, o_betas, root, trans)
            if p.has_offsets:
                x[219 * F + 10:] = p.offsets_start(x).reshape(-1)
            t = [p.time_closure(x, iters=a.iters) * 1e3 for _ in range(a.repeats)]
            line.append("%s %s us (median %.2f)" % (name, " ".join("%.1f" % v for v in t), np.median(t)))
        print("closure latent_offsets %-3s F=%d M=%d  %s" % (label, F, M, ";  ".join(line)))


if __name__ == "__main__":
    main()
