"""What the time_<term>.py tools share: the synthetic F x M case on the device, the three closure kinds of one configuration
(chamfer, one-hot marker, three-corner marker) and the alternating-rounds timing loop over several configurations
(uuo_time_closure through Problem.time_closure).  Each tool keeps its own configurations, labels and printed lines."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uuo_mocap_amd.body_model import synthetic_smpl  # noqa: E402
from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence  # noqa: E402

STAGES = ("chamfer", "marker", "marker3")


def stage_case(F, M, dev, **sequence_kw):
    """The synthetic model (`smpl`, `tables`), a make_sequence capture (seed 0; `sequence_kw` go to make_sequence) and the stage
    inputs on `dev`: markers, o_pose, o_betas, root, trans, the markers' vertices `vids` and a three-corner placement i3, b3
    (a face at each marker's vertex, weights of a third)."""
    c = types.SimpleNamespace(F=F, M=M, dev=dev)
    c.tables = synthetic_smpl(0)
    c.smpl = SmplInference(dev, tables=c.tables)
    c.seq = seq = make_sequence(c.tables, seed=0, num_frames=F, num_markers=M, **sequence_kw)
    c.markers = torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float().to(dev)
    c.o_pose = seq.img_smpl.pose_body.float().to(dev)
    c.o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).float().to(dev)
    c.root = seq.img_smpl.root_orient.float().to(dev)
    c.trans = torch.median(c.markers, dim=1)[0]
    c.vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32).to(dev)
    faces = torch.from_numpy(np.asarray(c.tables.faces).astype(np.int64))
    c.i3 = torch.stack([torch.sort(faces[(faces == int(v)).any(1).nonzero()[0, 0]])[0] for v in c.vids.cpu()]).to(torch.int32).to(dev)
    c.b3 = torch.full((M, 3), 1.0 / 3.0, device=dev)
    return c


def stage_problems(smpl, case, cfg, **kw):
    """The three closure kinds of `cfg` on the case; `kw` (a term's evidence) goes to every problem"""
    c = case
    return {
        "chamfer": ChamferProblem(smpl, c.markers, c.o_pose, c.o_betas, c.root, cfg, **kw),
        "marker": MarkerProblem(smpl, c.markers, c.o_pose, c.o_betas, c.vids, cfg, **kw),
        "marker3": MarkerProblem(smpl, c.markers, c.o_pose, c.o_betas, c.i3, cfg, bary=c.b3, **kw),
    }


def time_rounds(labels, probs, case, repeats, iters):
    """(label, stage) -> the `repeats` times in microseconds of one closure evaluation at the targets.  Alternating rounds: every
    configuration of `labels` once per repeat, so that a drift of the device's clocks falls on all of them alike."""
    c, times = case, {}
    for _ in range(repeats):
        for label in labels:
            for name, p in probs[label].items():
                x = p.pack(c.trans, torch.zeros(c.F, 1, 1, device=c.dev), c.o_betas, c.o_pose) if name == "chamfer" else \
                    p.pack(c.o_pose, c.o_betas, c.root, c.trans)
                times.setdefault((label, name), []).append(p.time_closure(x, iters=iters) * 1e3)
    return times
