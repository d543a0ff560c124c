"""Device time of one closure evaluation with the Geman-McClure data term off and on (uuo_time_closure), chamfer and marker
stages at F x M, and one whole fit per config.  python tools/time_robust.py [--frames 300 --markers 50]"""
import argparse
import copy
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uuo_mocap_amd.body_model import synthetic_smpl  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fits", type=int, default=2)
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
    for name in ("video_mocap", "video_mocap_robust"):
        cfg = packaged_config(name)
        pc = ChamferProblem(smpl, markers, o_pose, o_betas, root, cfg)
        xc = pc.pack(trans, torch.zeros(F, 1, 1, device=dev), o_betas, o_pose)
        pm = MarkerProblem(smpl, markers, o_pose, o_betas, vids, cfg)
        xm = pm.pack(o_pose, o_betas, root, trans)
        tc = [pc.time_closure(xc, iters=a.iters) * 1e3 for _ in range(a.repeats)]
        tm = [pm.time_closure(xm, iters=a.iters) * 1e3 for _ in range(a.repeats)]
        print("closure %-20s chamfer %s us  marker %s us  (median %.1f / %.1f)"
              % (name, " ".join("%.1f" % v for v in tc), " ".join("%.1f" % v for v in tm), np.median(tc), np.median(tm)))
    from uuo_mocap_amd.multimodal import multimodal_video_mocap

    for k in range(a.fits):
        for name in ("video_mocap", "video_mocap_robust"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(seq.markers.get_points().copy(), 30.0), dev,
                                   packaged_config(name), offset=0, print_options=[], save_stages=False, smpl_inference=smpl)
            torch.cuda.synchronize()
            print("fit %d %-20s %.3f s" % (k, name, time.perf_counter() - t0))


if __name__ == "__main__":
    main()
