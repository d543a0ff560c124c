"""Weight sweep of the pose-acceleration term on the local body rotations: fits the default 300 x 50
synthetic capture with video_mocap.yaml and with pose_accel weights over decades, and prints per setting the
rotation-acceleration error over the leaf joints (feet 10, 11, head 15, hands 22, 23) and over all 23 body joints, the
acceleration error of the joint positions and the mean vertex error.  --fused runs the term on the fused closures
(execution.pose_accel_fused: True), where the 25-pair sweep is cheap; without it the term runs composed.
python tools/sweep_pose_accel.py [--frames 300 --markers 50 --seed 0 --weights 0:0,1:0.1,10:1 --fused]"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.smpl_ref import SmplInferenceRef  # noqa: E402
from uuo_mocap_amd.body_model import synthetic_smpl  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.metrics import LEAF_JOINT_ROWS as LEAF_ROWS, compute_accel_error, compute_rotation_accel_error  # noqa: E402
from uuo_mocap_amd.multimodal import multimodal_video_mocap  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

DECADES = (0.1, 1.0, 10.0, 100.0, 1000.0)  # one value per decade for each stage, every pair
DEFAULT = "0:0," + ",".join("%g:%g" % (wc, wm) for wc in DECADES for wm in DECADES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", default=DEFAULT, help="chamfer:marker rows, comma separated; 0:0 is video_mocap.yaml")
    ap.add_argument("--fused", action="store_true", help="execution.pose_accel_fused: True (the fused closures)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tables = synthetic_smpl(0)
    smpl, ref = SmplInference(dev, tables=tables), SmplInferenceRef(tables)
    seq = make_sequence(tables, seed=a.seed, num_frames=a.frames, num_markers=a.markers)
    gt_rot = torch.from_numpy(np.asarray(seq.gt["rot"]))[:, 1:].double()
    gt_joints = torch.from_numpy(np.asarray(seq.gt["joints"]))[:, :24].double()
    gt_verts = torch.from_numpy(seq.gt["verts"])
    hmr = seq.img_smpl.pose_body.double()
    print("capture: %d x %d; the video's pose: rotation-acceleration error leaf %.2f all %.2f (30 Hz)"
          % (a.frames, a.markers, float(compute_rotation_accel_error(hmr, gt_rot, 30.0, LEAF_ROWS)),
             float(compute_rotation_accel_error(hmr, gt_rot, 30.0))), flush=True)
    rows = []
    for row in a.weights.split(","):
        wc, wm = (float(v) for v in row.split(":"))
        cfg = packaged_config("video_mocap")
        if a.fused:
            cfg["execution"] = dict(cfg.get("execution") or {}, pose_accel_fused=True)
        for stage, w in (("chamfer", wc), ("marker", wm)):
            if w:
                cfg["stages"][stage]["losses"]["pose_accel"] = w
        pts = np.asarray(seq.markers.get_points()).copy()
        out = multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(pts, 30.0), dev, copy.deepcopy(cfg), offset=0,
                                     print_options=[], save_stages=False, smpl_inference=smpl)
        r = ref(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                out["trans"].cpu().float())
        rot = out["pose_body"].cpu().double()
        leaf = float(compute_rotation_accel_error(rot, gt_rot, 30.0, LEAF_ROWS))
        every = float(compute_rotation_accel_error(rot, gt_rot, 30.0))
        acc = float(compute_accel_error(r["joints"][:, :24].double(), gt_joints, 30.0))
        verr = 1e3 * float((r["vertices"] - gt_verts).norm(dim=-1).mean())
        print("pose_accel %s | rotation accel leaf %.3f all %.3f | joint accel %.3f m/s^2 | vertex %.2f mm"
              % (row, leaf, every, acc, verr), flush=True)
        rows.append((row, leaf, verr))
    plain = [r for r in rows if r[0] == "0:0"]
    if plain:  # the rule of the extension configs: the lowest leaf-joint error within 0.5 mm of the plain fit's vertex error
        ok = [r for r in rows if r[0] != "0:0" and r[2] <= plain[0][2] + 0.5]
        print("rule: %s" % ("no setting qualifies" if not ok else "%s (leaf %.3f, vertex %.2f mm)" % min(ok, key=lambda r: r[1])))


if __name__ == "__main__":
    main()
