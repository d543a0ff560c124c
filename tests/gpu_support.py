"""What the GPU tests share: the device fixtures, the synthetic case every parity check evaluates, the problem makers, the fits
of the config tests and the weights at which one term's parity check switches another term on.  A test module imports the
fixtures by name (each importing module builds its own, module-scoped).  Importable without a GPU: only the fixtures need one."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (importable from tests/ without pytest's conftest)
    sys.path.insert(0, ROOT)
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

M = 50
# weights of the parity checks, per term (chamfer stage, marker stage): each term's own test states why its pair makes the term
# matter at _inputs' perturbations, the other terms' tests switch it on at the same weights
W_ACCEL_C, W_ACCEL_M = 10.0, 1.0      # joint_accel
W_LOCK_C, W_LOCK_M = 100.0, 10.0      # foot_lock
W_FLOOR_C, W_FLOOR_M = 100.0, 10.0    # floor_penetration / floor_contact
W_OFFS = 2.0                          # latent_offsets (marker stage)
W_CAPS_C, W_CAPS_M = 100.0, 10.0      # self_penetration
W_LIM_C, W_LIM_M = 10.0, 1.0          # joint_limits
R_CHAMFER, R_MARKER = 600.0, 60.0     # reg_pose_body where the weighted prior has to show (test_gpu_prior_confidence.py)
W_KP_C, W_KP_M = 0.05, 0.02           # keypoints_2d, pixels^-2
W_PACC_C, W_PACC_M = 1000.0, 1000.0   # pose_accel: video_mocap_rotsmooth.yaml's
U_TABLE = [1.0] * 23
U_TABLE[3], U_TABLE[9], U_TABLE[17] = 0.0, 0.5, 1.75    # tests/test_pose_accel.py's: a zero, a value below and one above 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def smpl(tables, dev):
    from uuo_mocap_amd.smpl import SmplInference

    return SmplInference(dev, tables=tables)


@pytest.fixture(scope="module")
def smpl64(tables):
    from oracle.smpl_ref import SmplInferenceRef

    return SmplInferenceRef(tables).double()


def _rel_err(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _check_grad(grad, g_ref, blocks, tag, record_property):
    """Whole vector < 2e-4 relative; each block < 5e-4 relative (or, when its float64 norm is below 1e-6 of the total,
    absolute error < 5e-4 x the total norm)."""
    grad, g_ref = np.asarray(grad, np.float64), np.asarray(g_ref, np.float64)
    assert np.isfinite(grad).all(), tag
    total = float(np.linalg.norm(g_ref))
    whole = _rel_err(grad, g_ref)
    record_property("grad_rel_%s" % tag, whole)
    msg = ["%s whole %.2e" % (tag, whole)]
    bad = []
    for name, sl in blocks:
        e, n = float(np.linalg.norm(grad[sl] - g_ref[sl])), float(np.linalg.norm(g_ref[sl]))
        if n < 1e-6 * total:
            msg.append("%s abs %.2e of total" % (name, e / total))
            if not e < 5e-4 * total:
                bad.append(name)
        else:
            msg.append("%s %.2e" % (name, e / n))
            record_property("grad_rel_%s_%s" % (tag, name), e / n)
            if not e / n < 5e-4:
                bad.append(name)
    print("; ".join(msg))
    assert whole < 2e-4 and not bad, "; ".join(msg)


# ------------------------------------------------------------------------------------------------ the case
def _inputs(tables, F, seed, num_markers=M):
    """A make_sequence capture and the point the closures are evaluated at: the targets perturbed (translation by 2 cm, yaw by
    0.3 rad, betas by 0.3, every rotation entry by 0.05), as (trans, z, betas, pose, root)"""
    seq = make_sequence(tables, seed=seed, num_frames=F, num_markers=num_markers)
    markers = torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float()
    o_pose = seq.img_smpl.pose_body.clone().float()
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).float()
    root = seq.img_smpl.root_orient.clone().float()
    trans = torch.median(markers, dim=1)[0].clone()
    gen = torch.Generator().manual_seed(seed + 2)
    r = lambda *s: torch.randn(*s, generator=gen)
    pert = (trans + 0.02 * r(F, 3), 0.3 * r(F, 1, 1), o_betas + 0.3 * r(1, 10), o_pose + 0.05 * r(F, 23, 3, 3),
            root + 0.05 * r(F, 1, 3, 3))
    return seq, markers, o_pose, o_betas, root, trans, pert


def _three_corners(tables, seq, seed, num_markers=M):
    """A three-corner placement per marker: a face at the marker's vertex (sorted ids) with random barycentric weights"""
    gen = torch.Generator().manual_seed(seed)
    faces = torch.from_numpy(np.asarray(tables.faces).astype(np.int64))
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    i3 = torch.zeros(num_markers, 3, dtype=torch.int64)
    b3 = torch.zeros(num_markers, 3)
    for m in range(num_markers):
        hit = (faces == vids[m]).any(1).nonzero()
        tri = faces[hit[0, 0]] if len(hit) else torch.tensor([int(vids[m]), (int(vids[m]) + 1) % 6890, (int(vids[m]) + 2) % 6890])
        wt = torch.rand(3, generator=gen) + 0.05
        i3[m], b3[m] = torch.sort(tri)[0], wt / wt.sum()
    return i3.to(torch.int32), b3


def _marker_x(pm, pp, bp, rp, tp, dev, seed, num_markers=M):
    """The marker problem's packed point, with random latent offsets of about MARKER_DISTANCE when the problem has them"""
    M = num_markers
    if not pm.has_offsets:
        return pm.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
    from uuo_mocap_amd.engine import MARKER_DISTANCE

    gen = torch.Generator().manual_seed(seed + 7)
    d = torch.randn(M, 3, generator=gen)
    offs = (MARKER_DISTANCE * (1.0 + 0.3 * torch.randn(M, 1, generator=gen))) * d / d.norm(dim=1, keepdim=True)
    return pm.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev), offs.to(dev))


# ------------------------------------------------------------------------------------------------ the three closure kinds
def _makers(smpl, dev, md, o_pose, o_betas, root, vids, i3, b3, pert):
    """name -> (make(cfg), pack(problem)) of the chamfer, the one-hot and the three-corner marker closure"""
    return {name: (lambda c, make=make: make(c, None), pack)
            for name, (make, pack) in _makers_contacts(smpl, dev, md, o_pose, o_betas, root, vids, i3, b3, pert).items()}


def _makers_contacts(smpl, dev, md, o_pose, o_betas, root, vids, i3, b3, pert):
    """name -> (make(cfg, foot_contacts), pack(problem)) of the chamfer, the one-hot and the three-corner marker closure"""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    tp, zp, bp, pp, rp = pert
    a = (md, o_pose.to(dev), o_betas.to(dev))
    return {
        "chamfer": (lambda c, fc: ChamferProblem(smpl, *a, root.to(dev), c, foot_contacts=fc),
                    lambda p: p.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))),
        "marker": (lambda c, fc: MarkerProblem(smpl, *a, vids.to(dev), c, foot_contacts=fc),
                   lambda p: p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))),
        "marker3": (lambda c, fc: MarkerProblem(smpl, *a, i3.to(dev), c, bary=b3.to(dev), foot_contacts=fc),
                    lambda p: p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))),
    }


# ------------------------------------------------------------------------------------------------ whole fits
def _fit_points(seq, points, cfg_name, smpl, dev, iters=None):
    """multimodal_video_mocap of a packaged config on the capture's video with the marker array `points`"""
    from uuo_mocap_amd.multimodal import multimodal_video_mocap

    cfg = packaged_config(cfg_name)
    if iters is not None:
        for k in ("chamfer", "marker", "part"):
            cfg["stages"][k]["num_iters"] = iters
    return multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(points.copy(), 30.0), dev, cfg, offset=0,
                                  print_options=[], save_stages=False, smpl_inference=smpl)


def _fit(seq, cfg_name, smpl, dev):
    return _fit_points(seq, np.asarray(seq.markers.get_points()), cfg_name, smpl, dev)


def _vertex_error(out, seq, oracle_smpl):
    r = oracle_smpl(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                    out["trans"].cpu().float())
    return float((r["vertices"] - torch.from_numpy(seq.gt["verts"])).norm(dim=-1).mean())
