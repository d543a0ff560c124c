"""Weight sweep of the floor-contact term on the capture with a floor: fits a 300 x 50 synthetic capture
with planted feet on a floor, with all markers and with the columns owned by joints 7, 8, 10, 11 removed, with video_mocap.yaml
and with floor weights over decades (a row's weight goes on floor_penetration and floor_contact alike; `p` / `c` keep one piece
only; `+lock` adds video_mocap_contact.yaml's foot_lock), and prints penetration and float against the true contacts, foot
skate and mean vertex error.
python tools/sweep_floor.py [--frames 300 --markers 50 --seed 0 --weights 100:10,1000:100+lock,100:10:p]"""
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
from uuo_mocap_amd.metrics import compute_floor_error, compute_foot_skate  # noqa: E402
from uuo_mocap_amd.multimodal import multimodal_video_mocap  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

DEFAULT = ("0:0,1:0.1,10:1,100:10,1000:100,10000:1000,100000:10000,0:0+lock,100:10+lock,1000:100+lock,10000:1000+lock,"
           "1000:100:p,1000:100:c")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", default=DEFAULT, help="chamfer:marker[:p|:c][+lock] rows, comma separated; 0:0 is video_mocap.yaml")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tables = synthetic_smpl(0)
    smpl, ref = SmplInference(dev, tables=tables), SmplInferenceRef(tables)
    seq = make_sequence(tables, seed=a.seed, num_frames=a.frames, num_markers=a.markers, planted_feet=True, floor=True)
    full = np.asarray(seq.markers.get_points())
    owner = np.argmax(np.asarray(tables.lbs_weights)[np.asarray(seq.gt["marker_vids"])], axis=1)
    keep = ~np.isin(owner, [7, 8, 10, 11])
    gt_v = torch.from_numpy(seq.gt["verts"])
    true_c = torch.from_numpy(seq.gt["foot_contacts"])
    sole = torch.from_numpy(np.asarray(seq.gt["sole_vids"]).reshape(-1).copy()).long()
    k_left = int(np.asarray(seq.gt["sole_vids"]).shape[1])
    lock = packaged_config("video_mocap_contact")
    print("capture: %d x %d, true contacts %s, seen %s" % (a.frames, a.markers, true_c.sum(0).tolist(),
                                                           seq.img_smpl.foot_contacts.sum(0).tolist()), flush=True)
    plain = {}
    for row in a.weights.split(","):
        spec, with_lock = (row[:-5], True) if row.endswith("+lock") else (row, False)
        parts = spec.split(":")
        wc, wm = float(parts[0]), float(parts[1])
        piece = parts[2] if len(parts) > 2 else "pc"
        cfg = packaged_config("video_mocap")
        for stage, w in (("chamfer", wc), ("marker", wm)):
            if w and "p" in piece:
                cfg["stages"][stage]["losses"]["floor_penetration"] = w
            if w and "c" in piece:
                cfg["stages"][stage]["losses"]["floor_contact"] = w
            if with_lock:
                cfg["stages"][stage]["losses"]["foot_lock"] = lock["stages"][stage]["losses"]["foot_lock"]
        out_row = []
        for tag, pts in (("all", full), ("no foot markers", full[:, keep])):
            out = multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(pts.copy(), 30.0), dev, copy.deepcopy(cfg),
                                         offset=0, print_options=[], save_stages=False, smpl_inference=smpl)
            r = ref(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                    out["trans"].cpu().float())
            e = compute_floor_error(r["vertices"][:, sole, 2], k_left, true_c, seq.gt["floor_height"])
            skate = float(compute_foot_skate(r["joints"][:, :24], true_c, 30.0))
            verr = 1e3 * float((r["vertices"] - gt_v).norm(dim=-1).mean())
            if wc == 0 and wm == 0 and not with_lock:
                plain[tag] = (e["penetration_mm"], e["float_mm"])
            rp = e["penetration_mm"] / plain[tag][0] if tag in plain and plain[tag][0] else float("nan")
            rf = e["float_mm"] / plain[tag][1] if tag in plain and plain[tag][1] else float("nan")
            out_row.append("%s (M=%d): pen %.3f mm (%.2f x) max %.1f mm float %.3f mm (%.2f x) skate %.3f m/s vertex %.2f mm"
                           % (tag, pts.shape[1], e["penetration_mm"], rp, e["max_penetration_mm"], e["float_mm"], rf, skate, verr))
        print("floor %s | %s" % (row, " | ".join(out_row)), flush=True)


if __name__ == "__main__":
    main()
