"""Sweep of the pose prior's confidence block: fits the 300 x 50 synthetic capture whose video loses the
person for 90 frames (make_sequence(video_dropout=True)) with video_mocap.yaml and with stages.{chamfer,marker}.prior_confidence
over gap_weight x ramp, and prints the mean vertex error inside and outside the window.  The rule of the shipped yaml: the pair
with the lowest in-window error whose out-of-window error stays within 0.5 mm of the plain fit's.
python tools/sweep_prior_confidence.py [--frames 300 --markers 50 --seed 0 --gap-weights 0,0.1,0.3 --ramps 0,5]"""
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
from uuo_mocap_amd.metrics import compute_window_vertex_error  # noqa: E402
from uuo_mocap_amd.multimodal import multimodal_video_mocap  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--gap-weights", default="0,0.1,0.3")
    ap.add_argument("--ramps", default="0,5")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tables = synthetic_smpl(0)
    smpl, ref = SmplInference(dev, tables=tables), SmplInferenceRef(tables)
    seq = make_sequence(tables, seed=a.seed, num_frames=a.frames, num_markers=a.markers, video_dropout=True)
    w0, w1 = seq.gt["dropout_window"]
    err = seq.gt["hmr_gap_error"]
    print("capture: %d x %d, window %d .. %d, filled target %.3f rad off there, stand-in %.3f rad elsewhere"
          % (a.frames, a.markers, w0, w1 - 1, err[w0:w1].mean(), np.concatenate([err[:w0], err[w1:]]).mean()), flush=True)
    rows = [None] + [(float(g), int(r)) for g in a.gap_weights.split(",") for r in a.ramps.split(",")]
    plain, best = None, None
    for row in rows:
        cfg = packaged_config("video_mocap")
        if row is not None:
            for stage in ("chamfer", "marker"):
                cfg["stages"][stage]["prior_confidence"] = {"gap_weight": row[0], "ramp": row[1], "joint_weights": None}
        out = multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(np.asarray(seq.markers.get_points()).copy(), 30.0),
                                     dev, cfg, offset=0, print_options=[], save_stages=False, smpl_inference=smpl)
        r = ref(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(), out["trans"].cpu().float())
        e = compute_window_vertex_error(r["vertices"], torch.from_numpy(seq.gt["verts"]), (w0, w1))
        if row is None:
            plain = e
        elif e["outside"] <= plain["outside"] + 5e-4 and (best is None or e["inside"] < best[1]["inside"]):
            best = (row, e)
        print("%-28s | vertex error inside %.2f mm, outside %.2f mm, all %.2f mm"
              % ("video_mocap.yaml" if row is None else "gap_weight %.2f ramp %d" % row, 1e3 * e["inside"], 1e3 * e["outside"],
                 1e3 * e["all"]), flush=True)
    if best is None or best[1]["inside"] >= plain["inside"]:
        print("no setting beats the plain fit inside the window within 0.5 mm outside it")
    else:
        print("rule's choice: gap_weight %.2f ramp %d (inside %.2f -> %.2f mm)"
              % (best[0][0], best[0][1], 1e3 * plain["inside"], 1e3 * best[1]["inside"]))


if __name__ == "__main__":
    main()
