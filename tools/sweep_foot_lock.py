"""Weight sweep of the foot-lock term on the planted-feet capture: fits a 300 x 50 synthetic capture with
planted feet, with all markers and with the columns owned by joints 7, 8, 10, 11 removed, with video_mocap.yaml and with
foot_lock weights over decades, and prints foot skate against the true contacts, mean vertex error and acceleration error.
python tools/sweep_foot_lock.py [--frames 300 --markers 50 --seed 0 --weights 30:10,100:30]"""
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
from uuo_mocap_amd.metrics import compute_accel_error, compute_foot_skate  # noqa: E402
from uuo_mocap_amd.multimodal import multimodal_video_mocap  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

DEFAULT = "0:0,3:1,10:3,30:10,100:30,300:100,1000:300,3000:1000,10000:3000,0:100,0:1000,100:0,1000:0,100:100,1000:1000"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", default=DEFAULT, help="chamfer:marker pairs, comma separated; 0:0 is video_mocap.yaml")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tables = synthetic_smpl(0)
    smpl, ref = SmplInference(dev, tables=tables), SmplInferenceRef(tables)
    seq = make_sequence(tables, seed=a.seed, num_frames=a.frames, num_markers=a.markers, planted_feet=True)
    full = np.asarray(seq.markers.get_points())
    owner = np.argmax(np.asarray(tables.lbs_weights)[np.asarray(seq.gt["marker_vids"])], axis=1)
    keep = ~np.isin(owner, [7, 8, 10, 11])
    gt_j = torch.from_numpy(np.asarray(seq.gt["joints"]))[:, :24].float()
    gt_v = torch.from_numpy(seq.gt["verts"])
    true_c = torch.from_numpy(seq.gt["foot_contacts"])
    plain = {}
    for pair in a.weights.split(","):
        wc, wm = (float(v) for v in pair.split(":"))
        cfg = packaged_config("video_mocap")
        if wc:
            cfg["stages"]["chamfer"]["losses"]["foot_lock"] = wc
        if wm:
            cfg["stages"]["marker"]["losses"]["foot_lock"] = wm
        row = []
        for tag, pts in (("all", full), ("no foot markers", full[:, keep])):
            out = multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(pts.copy(), 30.0), dev, copy.deepcopy(cfg),
                                         offset=0, print_options=[], save_stages=False, smpl_inference=smpl)
            r = ref(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                    out["trans"].cpu().float())
            j = r["joints"][:, :24]
            skate = float(compute_foot_skate(j, true_c, 30.0))
            verr = 1e3 * float((r["vertices"] - gt_v).norm(dim=-1).mean())
            acc = float(compute_accel_error(j, gt_j, 30.0))
            if wc == 0 and wm == 0:
                plain[tag] = skate
            ratio = skate / plain[tag] if tag in plain else float("nan")
            row.append("%s (M=%d): skate %.4f m/s (%.2f x) vertex %.2f mm accel %.2f m/s^2" % (tag, pts.shape[1], skate, ratio, verr, acc))
        print("foot_lock chamfer %g marker %g | %s" % (wc, wm, " | ".join(row)), flush=True)


if __name__ == "__main__":
    main()
