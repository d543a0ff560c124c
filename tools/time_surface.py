"""Device time of one chamfer-stage closure evaluation at F x M: the plain (nearest-vertex) closure, the point-to-surface closure
(uuo_fit_set_surface: k_ring_pick + k_surf_fwd + k_bwd_items_f) and the same term composed from the operators
(execution.surface_fused: False: SmplInference forward, uuo_nn_argmin + uuo_ring_closest_points, autograd backward), alternated in
one process; HIP-event medians.  The kernel split comes from running this under rocprofv3 --kernel-trace --stats with --no-composed.
python tools/time_surface.py [--frames 300 --markers 50]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uuo_mocap_amd.body_model import synthetic_smpl  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.engine import ChamferProblem  # noqa: E402
from uuo_mocap_amd.losses import surface_chamfer_distance  # noqa: E402
from uuo_mocap_amd.optimization import get_marker_mask  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence  # noqa: E402
from uuo_mocap_amd.transforms import compute_root_orient_z, normalize_rot  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-composed", action="store_true")
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
    cfgs = {"plain": packaged_config("video_mocap"), "surface": packaged_config("video_mocap_surface")}
    probs = {k: ChamferProblem(smpl, markers, o_pose, o_betas, root, c) for k, c in cfgs.items()}
    x = probs["plain"].pack(trans, torch.zeros(F, 1, 1, device=dev), o_betas, o_pose)
    st = cfgs["surface"]["stages"]["chamfer"]
    w, d0 = float(st["losses"]["surface_chamfer"]), float(st["surface_distance"])
    mask = get_marker_mask(markers)

    def composed_once():
        leaves = [t.clone().requires_grad_(True) for t in (trans, torch.zeros(F, 1, 1, device=dev), o_betas, o_pose)]
        t_, z_, b_, p_ = leaves
        out = smpl(poses=normalize_rot(p_), betas=torch.repeat_interleave(b_, dim=0, repeats=F),
                   root_orient=normalize_rot(compute_root_orient_z(z_) @ root), trans=t_)
        loss = surface_chamfer_distance(markers, out["vertices"], mask, smpl, d0)[0] * w + \
            torch.nn.functional.mse_loss(p_, o_pose) * st["losses"]["reg_pose_body"] + \
            torch.nn.functional.mse_loss(b_, o_betas) * st["losses"]["reg_betas"]
        loss.backward()

    def composed_ms(iters):
        composed_once()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            composed_once()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    times = {"plain": [], "surface": [], "composed": []}
    for _ in range(a.repeats):  # alternated: the three see the same clocks
        for k in ("plain", "surface"):
            times[k].append(probs[k].time_closure(x, iters=a.iters) * 1e3)
        if not a.no_composed:
            times["composed"].append(composed_ms(max(a.iters // 10, 5)) * 1e3)
    for k, v in times.items():
        if v:
            print("closure %-9s %s us  (median %.1f)" % (k, " ".join("%.1f" % t for t in v), np.median(v)))
    print("surface / plain %.3f" % (np.median(times["surface"]) / np.median(times["plain"])))
    if times["composed"]:
        print("composed / surface %.1f" % (np.median(times["composed"]) / np.median(times["surface"])))


if __name__ == "__main__":
    main()
