"""Weight sweep of the joint-angle limit term: fits the default 300 x 50 synthetic capture and the one whose
HMR start bends the left knee 0.5 rad backwards for 24 frames while the left leg's markers are missing
(make_sequence(joint_limits=True)), with video_mocap.yaml and with joint_limits weights over decades, and prints the limit
violation inside the window (over all frames on the default capture) and the mean vertex error over all frames.
python tools/sweep_joint_limits.py [--frames 300 --markers 50 --seed 0 --weights 0:0,1:0.1,10:1]"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.smpl_ref import SmplInferenceRef  # noqa: E402
from uuo_mocap_amd.body_model import smpl_joint_limits, synthetic_smpl  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.metrics import compute_joint_limit_violation  # noqa: E402
from uuo_mocap_amd.multimodal import multimodal_video_mocap  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

DEFAULT = "0:0,0.001:0.0001,0.01:0.001,0.1:0.01,1:0.1,10:1,100:10,1000:100"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", default=DEFAULT, help="chamfer:marker rows, comma separated; 0:0 is video_mocap.yaml")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tables = synthetic_smpl(0)
    smpl, ref = SmplInference(dev, tables=tables), SmplInferenceRef(tables)
    limits = smpl_joint_limits()
    seqs = (("default", make_sequence(tables, seed=a.seed, num_frames=a.frames, num_markers=a.markers)),
            ("limited", make_sequence(tables, seed=a.seed, num_frames=a.frames, num_markers=a.markers, joint_limits=True)))
    w0, w1 = seqs[1][1].gt["limit_window"]
    print("capture: %d x %d, window %d .. %d, HMR start's largest violation there %.1f deg (max)"
          % (a.frames, a.markers, w0, w1 - 1, float(np.degrees(seqs[1][1].gt["hmr_violation"][w0:w1].max()))), flush=True)
    plain = {}
    for row in a.weights.split(","):
        wc, wm = (float(v) for v in row.split(":"))
        cfg = packaged_config("video_mocap")
        for stage, w in (("chamfer", wc), ("marker", wm)):
            if w:
                cfg["stages"][stage]["losses"]["joint_limits"] = w
        out_row = []
        for tag, seq in seqs:
            pts = np.asarray(seq.markers.get_points()).copy()
            out = multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(pts, 30.0), dev, copy.deepcopy(cfg), offset=0,
                                         print_options=[], save_stages=False, smpl_inference=smpl)
            r = ref(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                    out["trans"].cpu().float())
            rot = out["pose_body"].cpu().float()
            e = compute_joint_limit_violation(rot[w0:w1] if tag == "limited" else rot, *limits)
            verr = 1e3 * float((r["vertices"] - torch.from_numpy(seq.gt["verts"])).norm(dim=-1).mean())
            if wc == 0 and wm == 0:
                plain[tag] = e["mean_deg"]
            ratio = e["mean_deg"] / plain[tag] if plain.get(tag) else float("nan")
            out_row.append("%s: violation mean %.3f deg (%.2f x) max %.2f deg frames %.0f %% vertex %.2f mm"
                           % (tag, e["mean_deg"], ratio, e["max_deg"], e["frames_pct"], verr))
        print("joint_limits %s | %s" % (row, " | ".join(out_row)), flush=True)


if __name__ == "__main__":
    main()
