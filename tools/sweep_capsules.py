"""Weight sweep of the bone-capsule self-penetration term: fits the default 300 x 50 synthetic capture and
the one whose HMR start has the left arm 30 mm inside the trunk for 24 frames while the arm's markers are missing
(make_sequence(self_penetration=True)), with video_mocap.yaml and with self_penetration weights over decades, and prints the
self-penetration inside the window (over all frames on the default capture) and the mean vertex error over all frames.
python tools/sweep_capsules.py [--frames 300 --markers 50 --seed 0 --weights 0:0,1:0.1,10:1]"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.smpl_ref import SmplInferenceRef  # noqa: E402
from uuo_mocap_amd.body_model import body_capsules, synthetic_smpl  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.metrics import compute_self_penetration  # noqa: E402
from uuo_mocap_amd.multimodal import multimodal_video_mocap  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

DEFAULT = "0:0,0.01:0.001,0.1:0.01,1:0.1,10:1,100:10,1000:100,10000:1000,100000:10000"


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
    caps = body_capsules(tables)
    seqs = (("default", make_sequence(tables, seed=a.seed, num_frames=a.frames, num_markers=a.markers)),
            ("penetrating", make_sequence(tables, seed=a.seed, num_frames=a.frames, num_markers=a.markers, self_penetration=True)))
    w0, w1 = seqs[1][1].gt["penetration_window"]
    print("capture: %d x %d, window %d .. %d, HMR start's arm / trunk overlap there %.1f mm (max)"
          % (a.frames, a.markers, w0, w1 - 1, 1e3 * float(seqs[1][1].gt["hmr_overlap"][w0:w1].max())), flush=True)
    plain = {}
    for row in a.weights.split(","):
        wc, wm = (float(v) for v in row.split(":"))
        cfg = packaged_config("video_mocap")
        for stage, w in (("chamfer", wc), ("marker", wm)):
            if w:
                cfg["stages"][stage]["losses"]["self_penetration"] = w
        out_row = []
        for tag, seq in seqs:
            pts = np.asarray(seq.markers.get_points()).copy()
            out = multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(pts, 30.0), dev, copy.deepcopy(cfg), offset=0,
                                         print_options=[], save_stages=False, smpl_inference=smpl)
            r = ref(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                    out["trans"].cpu().float())
            j = r["joints"][:, :24]
            e = compute_self_penetration(j[w0:w1] if tag == "penetrating" else j, *caps)
            verr = 1e3 * float((r["vertices"] - torch.from_numpy(seq.gt["verts"])).norm(dim=-1).mean())
            if wc == 0 and wm == 0:
                plain[tag] = e["mean_depth_mm"]
            ratio = e["mean_depth_mm"] / plain[tag] if plain.get(tag) else float("nan")
            out_row.append("%s: depth mean %.3f mm (%.2f x) max %.1f mm frames %.0f %% vertex %.2f mm"
                           % (tag, e["mean_depth_mm"], ratio, e["max_depth_mm"], e["frames_pct"], verr))
        print("self_penetration %s | %s" % (row, " | ".join(out_row)), flush=True)


if __name__ == "__main__":
    main()
