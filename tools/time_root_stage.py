"""Device time of one root-stage closure evaluation (uuo_time_closure), both packings, without and with trans_vel, beside the
part stage's full-skeleton closure of hmr_full.yaml (all vertices, one shared yaw, 1 / (F M)) and the chamfer closure, at F x M.
The configurations take turns inside every repeat (alternating rounds); the medians over the repeats are printed.
python tools/time_root_stage.py [--frames 300 --markers 50]"""
import argparse
import copy
import json

import numpy as np
import torch

from closure_case import stage_case  # (puts the repository on the path: keep it first)
from uuo_mocap_amd.config import packaged_config
from uuo_mocap_amd.engine import ChamferProblem, PartProblem, RootProblem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    F, M = a.frames, a.markers
    dev = torch.device("cuda:0")
    c = stage_case(F, M, dev)
    z1, zF = torch.zeros(1, 1, 1, device=dev), torch.zeros(F, 1, 1, device=dev)

    def root_cfg(shared, tvel):
        cfg = copy.deepcopy(packaged_config("video_mocap_root"))
        cfg["stages"]["root"].update(yaw_lock=not shared, constrained_rotation=shared)
        if tvel:
            cfg["stages"]["root"]["losses"]["trans_vel"] = tvel
        return cfg

    cases = {}
    for shared in (False, True):
        for tvel in (0.0, 1.0):
            p = RootProblem(c.smpl, c.markers, c.o_pose, c.o_betas, c.root, root_cfg(shared, tvel))
            cases["root_%s%s" % ("shared" if shared else "frame", "_tvel" if tvel else "")] = (p, p.pack(c.trans, z1 if shared else zF, c.o_betas))
    part = PartProblem(c.smpl, c.markers, c.o_pose, c.o_betas, c.root, torch.arange(c.smpl.device_model.V), packaged_config("hmr_full"))
    cases["part_full_skeleton"] = (part, part.pack(z1, c.trans, c.o_betas))
    ch = ChamferProblem(c.smpl, c.markers, c.o_pose, c.o_betas, c.root, packaged_config("video_mocap"))
    cases["chamfer"] = (ch, ch.pack(c.trans, zF, c.o_betas, c.o_pose))
    times = {k: [] for k in cases}
    for _ in range(a.repeats):
        for k, (p, x) in cases.items():
            times[k].append(p.time_closure(x, iters=a.iters) * 1e3)
    for k, v in times.items():
        print("closure %-20s F=%d M=%d  %s us (median %.2f)" % (k, F, M, " ".join("%.1f" % t for t in v), np.median(v)))
    print(json.dumps({"F": F, "M": M, "median_us": {k: round(float(np.median(v)), 2) for k, v in times.items()}}))


if __name__ == "__main__":
    main()
