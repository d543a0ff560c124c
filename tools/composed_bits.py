"""A/B of the stage solvers' host layer: optim_chamfer, then optim_markers from its result, on a 6 x 8 synthetic capture for the
plain config and every packaged extension config, each with the term's execution switch True (the fused closure) and False (the
closure composed from the operators).  One line per solve with last_stats' n_eval, n_iter and the first and final loss as
float.hex(): run it on two commits (twice each) and diff the output.  The first loss is one forward evaluation and must agree
bit for bit; the rest of a composed solve may move where a commit's own two runs already differ (atomics in an autograd
backward).  video_mocap_tracklets is left out (its per-frame table has no composed closure).
python tools/composed_bits.py [--iters 40]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uuo_mocap_amd.body_model import synthetic_smpl  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.engine import prior_weight_table, stage_prior_confidence  # noqa: E402
from uuo_mocap_amd.optimization import last_stats, optim_chamfer, optim_markers  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence  # noqa: E402

#: packaged config -> its execution switch (None: the config has one route only)
CONFIGS = (("video_mocap", None), ("video_mocap_robust", "robust_fused"), ("video_mocap_smooth", "temporal_fused"),
           ("video_mocap_offsets", None), ("video_mocap_contact", "temporal_fused"), ("video_mocap_floor", "floor_fused"),
           ("video_mocap_capsules", "capsule_fused"), ("video_mocap_limits", "limit_fused"),
           ("video_mocap_dropout", "prior_conf_fused"), ("video_mocap_rotsmooth", None), ("video_mocap_surface", "surface_fused"),
           ("video_mocap_soft", "chamfer_soft_fused"))
F, M = 6, 8


def _line(tag, st):
    first, final = (st[k] for k in (("loss_first", "loss_final") if "loss_first" in st else ("first_loss", "final_loss")))
    print("%-44s n_eval %4d n_iter %4d first %s final %s" % (tag, st["n_eval"], st["n_iter"], float(first).hex(), float(final).hex()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tables = synthetic_smpl(0)
    smpl = SmplInference(dev, tables=tables)
    seq = make_sequence(tables, seed=11, num_frames=F, num_markers=M)
    markers = torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float().to(dev)
    o_pose = seq.img_smpl.pose_body.float().to(dev)
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).float().to(dev)
    root = seq.img_smpl.root_orient.float()
    trans = torch.median(markers, dim=1)[0]
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long().to(dev)] = 1.0
    contacts = torch.zeros(F, 2)
    contacts[1:4, 0] = 1.0
    seen = torch.tensor([1, 1, 0, 0, 1, 1])
    mask, labels = torch.ones(F, device=dev), torch.zeros(F, M, dtype=torch.long, device=dev)
    for name, switch in CONFIGS:
        for fused in ((True, False) if switch else (True,)):
            cfg = packaged_config(name)
            for stage in ("chamfer", "marker"):
                cfg["stages"][stage]["num_iters"] = a.iters
            if switch:
                cfg["execution"] = {switch: fused}
            weights = {s: None if stage_prior_confidence(cfg, s) is None else prior_weight_table(seen, stage_prior_confidence(cfg, s))
                       for s in ("chamfer", "marker")}
            pose, betas, rt, tr = (t.clone().to(dev).requires_grad_(True) for t in (o_pose, o_betas, root, trans))
            tag = "%s %s=%s" % (name, switch, fused)
            optim_chamfer(markers, pose, o_pose, betas, o_betas, rt, tr, mask, labels, smpl, cfg, foot_contacts=contacts,
                          prior_weights=weights["chamfer"])
            _line(tag + " chamfer", last_stats("chamfer"))
            optim_markers(markers, pose, o_pose, betas, o_betas, rt, tr, one_hot, mask, smpl, cfg, foot_contacts=contacts,
                          prior_weights=weights["marker"])
            _line(tag + " marker", last_stats("marker"))


if __name__ == "__main__":
    main()
