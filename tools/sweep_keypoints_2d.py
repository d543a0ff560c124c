"""Weight sweep of the 2D key-point reprojection term: fits the 300 x 50 synthetic capture whose HMR start has
the left forearm turned 0.5 rad about the camera's depth axis for 24 frames while the arm's markers are missing
(make_sequence(elbow_error=True)), with video_mocap.yaml and with keypoints_2d weights over decades, at sigma 0 and at a
Geman-McClure scale, on synthetic_keypoints_2d of the capture (ground-truth joints through a fixed camera four metres away, 2 px
of noise).  Prints the mean position error of the left elbow's and wrist's joints (18, 20) inside the window and the mean vertex
error over all frames, and the setting the rule picks: among those that end within 0.5 mm of the plain fit's vertex error, the
lowest window error.
python tools/sweep_keypoints_2d.py [--frames 300 --markers 50 --seed 0 --weights 0:0,1e-4:1e-5 --sigmas 0,30]"""
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
from uuo_mocap_amd.multimodal import multimodal_video_mocap  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence, synthetic_keypoints_2d  # noqa: E402

DEFAULT = "0:0,1e-5:1e-6,1e-4:1e-5,1e-3:1e-4,1e-2:1e-3,1e-1:1e-2,1:1e-1"
ARM = (18, 20)  # left elbow, left wrist


def fit_errors(seq, cfg, rec, smpl, ref, dev):
    """(window's mean elbow and wrist error in mm, mean vertex error in mm) of one fit"""
    pts = np.asarray(seq.markers.get_points()).copy()
    out = multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(pts, 30.0), dev, copy.deepcopy(cfg), offset=0,
                                 print_options=[], save_stages=False, smpl_inference=smpl, keypoints_2d=rec)
    r = ref(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(), out["trans"].cpu().float())
    w0, w1 = seq.gt["elbow_window"]
    gt_j = torch.from_numpy(seq.gt["joints"])[w0:w1][:, list(ARM)]
    arm = 1e3 * float((r["joints"][w0:w1][:, list(ARM)] - gt_j).norm(dim=-1).mean())
    verr = 1e3 * float((r["vertices"] - torch.from_numpy(seq.gt["verts"])).norm(dim=-1).mean())
    return arm, verr


def keyed_config(wc, wm, sigma):
    cfg = packaged_config("video_mocap")
    for stage, w in (("chamfer", wc), ("marker", wm)):
        if w:
            cfg["stages"][stage]["losses"]["keypoints_2d"] = w
            cfg["stages"][stage]["keypoints_2d"] = {"sigma": sigma, "min_depth": 0.1, "joint_weights": None}
    return cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise", type=float, default=2.0)
    ap.add_argument("--weights", default=DEFAULT, help="chamfer:marker rows, comma separated; 0:0 is video_mocap.yaml")
    ap.add_argument("--sigmas", default="0,30", help="Geman-McClure scales in pixels, comma separated (0 = the square)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tables = synthetic_smpl(0)
    smpl, ref = SmplInference(dev, tables=tables), SmplInferenceRef(tables)
    seq = make_sequence(tables, seed=a.seed, num_frames=a.frames, num_markers=a.markers, elbow_error=True)
    rec = synthetic_keypoints_2d(seq, noise=a.noise, seed=a.seed)
    w0, w1 = seq.gt["elbow_window"]
    print("capture: %d x %d seed %d, window %d .. %d, key points: ground truth through a fixed camera, %.1f px noise"
          % (a.frames, a.markers, a.seed, w0, w1 - 1, a.noise), flush=True)
    rows, plain = [], None
    for row in a.weights.split(","):
        wc, wm = (float(v) for v in row.split(":"))
        for sigma in ([0.0] if wc == 0 and wm == 0 else [float(s) for s in a.sigmas.split(",")]):
            arm, verr = fit_errors(seq, keyed_config(wc, wm, sigma), rec if (wc or wm) else None, smpl, ref, dev)
            if wc == 0 and wm == 0:
                plain = (arm, verr)
            rows.append((row, sigma, arm, verr))
            print("keypoints_2d %s sigma %g | elbow + wrist in the window %.2f mm | vertex %.3f mm" % (row, sigma, arm, verr), flush=True)
    if plain is not None:
        ok = [r for r in rows if r[3] <= plain[1] + 0.5]
        best = min(ok, key=lambda r: r[2])
        print("rule (within 0.5 mm of the plain fit's %.3f mm, lowest window error): %s sigma %g -> %.2f mm (plain %.2f mm), vertex %.3f mm"
              % (plain[1], best[0], best[1], best[2], plain[0], best[3]))


if __name__ == "__main__":
    main()
