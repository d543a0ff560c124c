"""Device time (HIP events) of the two kernels of the tracklet placement beside the ones they stand next to: the marker closure
on a per-frame vertex table (uuo_fit_set_frame_assign) against the plain per-column marker closure, and the segmented placement
kernel (uuo_assign_segments_argmin) against uuo_assign_mean_argmin on the same inputs with one tracklet per column.  A build
without the extension prints the plain numbers only, so two builds can be alternated on one box.
python tools/time_tracklets.py [--frames 300 --markers 50]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uuo_mocap_amd.body_model import synthetic_smpl  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.engine import MarkerProblem  # noqa: E402
from uuo_mocap_amd.smpl import SmplInference  # noqa: E402
from uuo_mocap_amd.synthetic import make_sequence  # noqa: E402


def event_us(fn, iters, repeats):
    """`repeats` timings of `iters` back-to-back calls of fn, microseconds per call."""
    out = []
    fn()
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--markers", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tables = synthetic_smpl(0)
    smpl = SmplInference(dev, tables=tables)
    dm = smpl.device_model
    F, M = a.frames, a.markers
    has_ext = hasattr(dm, "assign_segments_argmin")
    seq = make_sequence(tables, seed=0, num_frames=F, num_markers=M)
    markers = torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float().to(dev)
    o_pose = seq.img_smpl.pose_body.float().to(dev)
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).float().to(dev)
    root = seq.img_smpl.root_orient.float().to(dev)
    trans = torch.median(markers, dim=1)[0]
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32).to(dev)
    tabs = {}
    if has_ext:
        ev = make_sequence(tables, seed=0, num_frames=F, num_markers=M, identity_events=12)
        tabs = {"constant table": vids[None, :].repeat(F, 1),
                "12-event table": torch.from_numpy(ev.gt["marker_vids_fm"]).to(torch.int32).to(dev)}
    fmt = lambda t: "%s us (median %.2f)" % (" ".join("%.1f" % v for v in t), np.median(t))  # noqa: E731
    smooth = packaged_config("video_mocap_smooth")
    robust = packaged_config("video_mocap_robust")
    for label, cfg in (("plain", packaged_config("video_mocap")), ("robust", robust), ("joint_accel", smooth)):
        probs = {"per-column": MarkerProblem(smpl, markers, o_pose, o_betas, vids, cfg)}
        for name, tab in tabs.items():
            probs[name] = MarkerProblem(smpl, markers, o_pose, o_betas, None, cfg, frame_assign=tab)
        line = []
        for name, p in probs.items():
            x = p.pack(o_pose, o_betas, root, trans)
            t = [p.time_closure(x, iters=a.iters) * 1e3 for _ in range(a.repeats)]
            line.append("%s %s" % (name, fmt(t)))
        print("marker closure %-12s F=%d M=%d  %s" % (label, F, M, ";  ".join(line)))
    with torch.no_grad():
        verts = smpl(poses=o_pose, betas=o_betas.expand(F, 10).contiguous(), root_orient=root, trans=trans)["vertices"].contiguous()
    valid = torch.ones(F, dtype=torch.bool, device=dev)
    line = ["uuo_assign_mean_argmin %s" % fmt(event_us(lambda: dm.assign_mean_argmin(verts, markers, valid), a.iters, a.repeats))]
    if has_ext:
        seg = torch.arange(M, dtype=torch.int32, device=dev)[None, :].expand(F, M).contiguous()
        valid_u8 = valid.to(torch.uint8)
        line.append("uuo_assign_segments_argmin, one tracklet per column %s"
                    % fmt(event_us(lambda: dm.assign_segments_argmin(verts, markers, seg, valid_u8, M), a.iters, a.repeats)))
        from uuo_mocap_amd.tracklets import tracklets_from_identity

        trk = tracklets_from_identity(torch.from_numpy(ev.gt["tracklets_fm"]), 10)
        seg_e = trk.seg.to(dev)
        mk_e = torch.from_numpy(ev.markers.get_points()).float().to(dev)
        line.append("12-event capture, %d tracklets %s"
                    % (trk.count, fmt(event_us(lambda: dm.assign_segments_argmin(verts, mk_e, seg_e, valid_u8, trk.count), a.iters,
                                               a.repeats))))
    print("placement F=%d M=%d V=%d (one call: memset + kernel + unpack; the per-column call also reads `valid` back)  %s"
          % (F, M, verts.shape[1], ";  ".join(line)))


if __name__ == "__main__":
    main()
