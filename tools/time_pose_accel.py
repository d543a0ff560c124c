"""Device time of one closure evaluation with the fused pose-acceleration term (k_pose_accel), beside the
plain closures and -- the yardstick, in the same call -- the joint-angle limit term's (k_limit_fwd, the kernel whose shape it
has): chamfer and marker (one-hot and three-corner) stages at F x M (uuo_time_closure).  The configurations take turns inside
every repeat (alternating rounds), and the medians over the repeats are printed with each term's increment over the plain
closure.  With --fit, one full fit of the capture with video_mocap_rotsmooth_fused.yaml follows (wall time after a warm-up fit
of video_mocap.yaml), and with --composed the same fit with video_mocap_rotsmooth.yaml, the term on the composed closures.
python tools/time_pose_accel.py [--frames 300 --markers 50] [--fit] [--composed]"""
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
    fused = packaged_config("video_mocap_rotsmooth_fused")
    both = packaged_config("video_mocap_limits")
    both["execution"] = dict(both.get("execution") or {}, pose_accel_fused=True)
    for k in ("chamfer", "marker"):
        both["stages"][k]["losses"]["pose_accel"] = fused["stages"][k]["losses"]["pose_accel"]
    labels = (("plain", packaged_config("video_mocap")), ("joint_limits", packaged_config("video_mocap_limits")),
              ("pose_accel", fused), ("pose_accel+joint_limits", both))
    probs, times = {}, {}
    for label, cfg in labels:
        probs[label] = {
            "chamfer": ChamferProblem(smpl, markers, o_pose, o_betas, root, cfg),
            "marker": MarkerProblem(smpl, markers, o_pose, o_betas, vids, cfg),
            "marker3": MarkerProblem(smpl, markers, o_pose, o_betas, i3, cfg, bary=b3),
        }
        assert all(p.pose_accel_on == label.startswith("pose_accel") for p in probs[label].values())
    for _ in range(a.repeats):  # alternating rounds: every configuration once per repeat
        for label, _cfg in labels:
            for name, p in probs[label].items():
                x = p.pack(trans, torch.zeros(F, 1, 1, device=dev), o_betas, o_pose) if name == "chamfer" else \
                    p.pack(o_pose, o_betas, root, trans)
                times.setdefault((label, name), []).append(p.time_closure(x, iters=a.iters) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for label, _cfg in labels:
        line = ["%s %s us (median %.2f, %+.2f over plain)" % (name, " ".join("%.1f" % v for v in times[(label, name)]),
                                                              med[(label, name)], med[(label, name)] - med[("plain", name)])
                for name in ("chamfer", "marker", "marker3")]
        print("closure %-24s F=%d M=%d  %s" % (label, F, M, ";  ".join(line)))
    if a.fit or a.composed:
        _fit(seq, "video_mocap", smpl, dev)  # warm-up: workspaces, the first launches
        names = ["video_mocap"] + (["video_mocap_rotsmooth_fused"] if a.fit else []) + (["video_mocap_rotsmooth"] if a.composed else [])
        for name in names:
            print("fit %-30s F=%d M=%d  %.2f s" % (name, F, M, _fit(seq, name, smpl, dev)), flush=True)


if __name__ == "__main__":
    main()
