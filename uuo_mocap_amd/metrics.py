"""Evaluation metrics with the reference's names and definitions (reference src/video_mocap/evaluation/metrics.py:27-190):
marker-to-surface distance (m2s), MPJPE / MPJVE and their Procrustes-aligned variants, V2V.  All of them run on the
tensors' device; m2s is the one with real work -- the closest point on the body surface for every marker and frame --
and uses the same HIP kernel as the barycentric marker placement (`uuo_mesh_closest_points`) where the reference
loops over frames calling igl.signed_distance."""
from __future__ import annotations

from typing import Dict, List

import numpy as np
import torch


def compute_marker_to_surface_distance(vertices: torch.Tensor, faces: torch.Tensor, markers: torch.Tensor) -> torch.Tensor:
    """mean_{f,m} |distance(markers[f,m], mesh(vertices[f], faces))| (metrics.py:27-45).  vertices [F,V,3], markers
    [F,M,3]; faces [NF,3] or the reference's per-frame [F,NF,3] (the first frame's list is used: one topology)."""
    from .engine import mesh_closest_points

    if faces.dim() == 3:
        if faces.shape[0] > 1 and not bool((faces == faces[:1]).all()):
            raise ValueError("per-frame face lists must share one topology")
        faces = faces[0]
    dist = mesh_closest_points(vertices, faces, markers)[0]
    return torch.mean(dist.double()).cpu()


def compute_MPJPE(pred_joints: torch.Tensor, gt_joints: torch.Tensor) -> torch.Tensor:
    return torch.mean(torch.norm(pred_joints - gt_joints, dim=-1))


def compute_MPJPE_joints(pred_joints: torch.Tensor, gt_joints: torch.Tensor, joints_ids: List[int]) -> torch.Tensor:
    return torch.mean(torch.norm(pred_joints[:, joints_ids] - gt_joints[:, joints_ids], dim=-1))


def _velocity_error(pred: torch.Tensor, gt: torch.Tensor, freq: float, joints_ids=None) -> torch.Tensor:
    pred_vel = (pred[1:] - pred[:-1]) * freq
    gt_vel = (gt[1:] - gt[:-1]) * freq
    if joints_ids is not None:
        pred_vel, gt_vel = pred_vel[:, joints_ids], gt_vel[:, joints_ids]
    return torch.mean(torch.norm(pred_vel - gt_vel, dim=-1))


def compute_MPJVE(pred_joints: torch.Tensor, gt_joints: torch.Tensor, freq: float) -> torch.Tensor:
    return _velocity_error(pred_joints, gt_joints, freq)


def compute_MPJVE_joints(pred_joints: torch.Tensor, gt_joints: torch.Tensor, freq: float,
                         joints_ids: List[int]) -> torch.Tensor:
    return _velocity_error(pred_joints, gt_joints, freq, joints_ids)


def compute_accel_error(pred_joints: torch.Tensor, gt_joints: torch.Tensor, freq: float) -> torch.Tensor:
    """Acceleration error (HMMR's "accel error"; not a metric of the reference): mean over frames 1 .. F-2 and joints of
    |a_pred - a_gt|, a_t = (x_{t-1} - 2 x_t + x_{t+1}) freq^2, in m/s^2 for positions in metres and `freq` in frames per
    second.  pred_joints, gt_joints [F, J, 3] with F >= 3."""
    if pred_joints.shape != gt_joints.shape or pred_joints.dim() != 3 or pred_joints.shape[0] < 3:
        raise ValueError("compute_accel_error: joints [F, J, 3] of equal shape with F >= 3 expected (got %s and %s)"
                         % (tuple(pred_joints.shape), tuple(gt_joints.shape)))
    accel = lambda x: (x[:-2] - 2.0 * x[1:-1] + x[2:]) * (float(freq) ** 2)
    return torch.mean(torch.norm(accel(pred_joints) - accel(gt_joints), dim=-1))


#: rows of a [F, 23, 3, 3] table of body rotations that hold the joints without a child: SMPL joints 10, 11 (feet), 15 (head),
#: 22, 23 (hands) -- row j - 1 is joint j
LEAF_JOINT_ROWS = (9, 10, 14, 21, 22)


def compute_rotation_accel_error(pred_rot: torch.Tensor, gt_rot: torch.Tensor, freq: float, joints_ids=None) -> torch.Tensor:
    """Rotation-acceleration error (not a metric of the reference): mean over frames 0 .. F-3 and joints of
    |(P_t - 2 P_{t+1} + P_{t+2}) - (G_t - 2 G_{t+1} + G_{t+2})|_F freq^2, the chordal second difference of the local rotations
    the pose-acceleration term acts on -- for small angles |R_a - R_b|_F is sqrt(2) times the angle, so the unit is about
    sqrt(2) rad/s^2 for `freq` in frames per second.  pred_rot, gt_rot [F, J, 3, 3] with F >= 3; `joints_ids` selects ROWS of
    the second dimension (for body rotations [F, 23, 3, 3] row j - 1 is SMPL joint j), None = all."""
    if pred_rot.shape != gt_rot.shape or pred_rot.dim() != 4 or tuple(pred_rot.shape[2:]) != (3, 3) or pred_rot.shape[0] < 3:
        raise ValueError("compute_rotation_accel_error: rotations [F, J, 3, 3] of equal shape with F >= 3 expected (got %s and %s)"
                         % (tuple(pred_rot.shape), tuple(gt_rot.shape)))
    if joints_ids is not None:
        ids = [int(j) for j in joints_ids]
        pred_rot, gt_rot = pred_rot[:, ids], gt_rot[:, ids]
    accel = lambda x: x[:-2] - 2.0 * x[1:-1] + x[2:]
    d = accel(pred_rot) - accel(gt_rot)
    return torch.mean(torch.sqrt((d * d).sum(dim=(-1, -2)))) * (float(freq) ** 2)


def compute_foot_skate(joints: torch.Tensor, contacts: torch.Tensor, freq: float) -> torch.Tensor:
    """Foot skate (not a metric of the reference): mean speed |J_t - J_{t-1}| freq of the feet (joints 10 and 11) over the
    (t, foot) pairs in contact in both frames (c_t c_{t-1} = 1), in m/s for positions in metres and `freq` in frames per
    second.  joints [F, >= 24, 3], contacts [F, 2] (left, right).  0.0 when no pair is in contact."""
    if joints.dim() != 3 or joints.shape[1] < 24 or joints.shape[2] != 3 or tuple(contacts.shape) != (joints.shape[0], 2):
        raise ValueError("compute_foot_skate: joints [F, >= 24, 3] and contacts [F, 2] expected (got %s and %s)"
                         % (tuple(joints.shape), tuple(contacts.shape)))
    if joints.shape[0] < 2:
        return joints.new_zeros(())
    contacts = contacts.to(device=joints.device, dtype=joints.dtype)
    gate = (contacts[1:] * contacts[:-1]) == 1.0
    if not bool(gate.any()):
        return joints.new_zeros(())
    speed = torch.norm(joints[1:, 10:12] - joints[:-1, 10:12], dim=-1) * float(freq)
    return speed[gate].mean()


def compute_floor_error(sole_z: torch.Tensor, k_left: int, contacts: torch.Tensor, height: float = 0.0) -> Dict[str, float]:
    """Floor errors (not metrics of the reference) of sole heights sole_z [F, K] (world z of the K sole points, the left foot's
    `k_left` first) against a plane at `height`, with contact labels contacts [F, 2] (left, right), in millimetres for heights
    in metres: `penetration_mm` the mean of max(h - z, 0) over all (t, p), `max_penetration_mm` its maximum, `float_mm` the mean
    of max(min_{p of foot s} z - h, 0) over the (t, s) with c = 1 (0.0 when there are none)."""
    k_left = int(k_left)
    if sole_z.dim() != 2 or not 0 < k_left < sole_z.shape[1] or tuple(contacts.shape) != (sole_z.shape[0], 2):
        raise ValueError("compute_floor_error: sole_z [F, K], 0 < k_left < K and contacts [F, 2] expected (got %s, %d and %s)"
                         % (tuple(sole_z.shape), k_left, tuple(contacts.shape)))
    z = sole_z.double()
    pen = torch.relu(float(height) - z)
    low = torch.stack([z[:, :k_left].min(dim=1).values, z[:, k_left:].min(dim=1).values], dim=1)
    flo = torch.relu(low - float(height))
    gate = contacts.to(device=z.device) == 1.0
    return {"penetration_mm": float(pen.mean()) * 1e3, "max_penetration_mm": float(pen.max()) * 1e3,
            "float_mm": float(flo[gate].mean()) * 1e3 if bool(gate.any()) else 0.0}


def compute_self_penetration(joints: torch.Tensor, cap_joints, cap_geom, pairs) -> Dict[str, float]:
    """Self-penetration (not a metric of the reference) of joints [F, >= 24, 3] under the capsule set of the self-penetration
    term (cap_joints [C, 2], cap_geom [C, 3], pairs [P, 2]; body_model.body_capsules builds the default), float64, in
    millimetres for joints in metres: `max_depth_mm` the deepest overlap max(r_i + r_j - d, 0) of any pair in any frame,
    `mean_depth_mm` the mean over frames of the frame's deepest pair, `frames_pct` the share of frames with any overlap."""
    from .body_model import capsule_pair_depths

    if joints.dim() != 3 or joints.shape[1] < 24 or joints.shape[2] != 3:
        raise ValueError("compute_self_penetration: joints [F, >= 24, 3] expected (got %s)" % (tuple(joints.shape),))
    pen = capsule_pair_depths(joints.detach().cpu().double().numpy(), cap_joints, cap_geom, pairs)
    deepest = pen.max(axis=1)
    return {"max_depth_mm": float(deepest.max()) * 1e3, "mean_depth_mm": float(deepest.mean()) * 1e3,
            "frames_pct": 100.0 * float((deepest > 0.0).mean())}


def compute_joint_limit_violation(rot_body: torch.Tensor, lo, hi) -> Dict[str, float]:
    """Joint-limit violation (not a metric of the reference) of body rotations [F, 23, 3, 3] under the tables of the joint-angle
    limit term (lo / hi [23, 3], radians; body_model.smpl_joint_limits builds the default), float64, in degrees: `max_deg` the
    largest pen = max(omega - hi, 0) + max(lo - omega, 0) of any component of any joint in any frame, `mean_deg` the mean over
    frames of the frame's largest pen, `frames_pct` the share of frames with any violation."""
    from .body_model import joint_limit_violation

    if rot_body.dim() != 4 or tuple(rot_body.shape[1:]) != (23, 3, 3):
        raise ValueError("compute_joint_limit_violation: rot_body [F, 23, 3, 3] expected (got %s)" % (tuple(rot_body.shape),))
    pen = joint_limit_violation(rot_body.detach().cpu().double().numpy(), lo, hi)
    worst = np.degrees(pen.reshape(pen.shape[0], -1).max(axis=1))
    return {"max_deg": float(worst.max()), "mean_deg": float(worst.mean()), "frames_pct": 100.0 * float((worst > 0.0).mean())}


def compute_pose_gmm_energy(rot_body: torch.Tensor, mixture: Dict) -> Dict:
    """EXTENSION: the mixture pose prior's energy (not a metric of the reference) of body rotations [F, 23, 3, 3] under `mixture`
    {means [K, 69], covars [K, 69, 69], weights [K]} (body_model.load_pose_mixture, synthetic.pose_mixture), float64, in nats:
    E_t = min_k 1/2 |A_k^T (theta_t - mu_k)|^2 + b_k with the offsets shifted so that the least is 0 (uuo_fit_set_pose_gmm).
    `mean` and `max` over the frames, `winner` [F] the winning component of every frame (ties: the lowest k)."""
    from .body_model import check_pose_mixture, pose_log_vector, pose_mixture_factors

    if rot_body.dim() != 4 or tuple(rot_body.shape[1:]) != (23, 3, 3):
        raise ValueError("compute_pose_gmm_energy: rot_body [F, 23, 3, 3] expected (got %s)" % (tuple(rot_body.shape),))
    mu, chol, off = pose_mixture_factors(*check_pose_mixture(mixture["means"], mixture["covars"], mixture["weights"],
                                                             "compute_pose_gmm_energy"))
    theta = pose_log_vector(rot_body.detach().cpu().double().numpy())
    y = np.einsum("krc,fkr->fkc", chol, theta[:, None, :] - mu[None])
    e = 0.5 * (y * y).sum(-1) + off[None]
    return {"mean": float(e.min(axis=1).mean()), "max": float(e.min(axis=1).max()), "winner": np.argmin(e, axis=1)}


def compute_window_vertex_error(pred_vertices: torch.Tensor, gt_vertices: torch.Tensor, window) -> Dict[str, float]:
    """EXTENSION: the mean vertex error (the tensors' unit) inside and outside the frame window (first frame, one past the
    last) -- what the pose prior's weights buy where the video lost the person, and what they cost elsewhere.  [F, V, 3] each;
    `inside` / `outside` are NaN when the window holds no / every frame."""
    if pred_vertices.dim() != 3 or tuple(pred_vertices.shape) != tuple(gt_vertices.shape):
        raise ValueError("compute_window_vertex_error: two [F, V, 3] tensors expected")
    w0, w1 = int(window[0]), int(window[1])
    F = int(pred_vertices.shape[0])
    if not 0 <= w0 <= w1 <= F:
        raise ValueError("compute_window_vertex_error: the window %r does not lie in the %d frames" % (window, F))
    e = (pred_vertices.detach().cpu().double() - gt_vertices.detach().cpu().double()).norm(dim=-1).mean(dim=1)
    inside = torch.zeros(F, dtype=torch.bool)
    inside[w0:w1] = True
    mean = lambda v: float(v.mean()) if v.numel() else float("nan")
    return {"inside": mean(e[inside]), "outside": mean(e[~inside]), "all": mean(e)}


def compute_PA_MPJPE(pred_joints: torch.Tensor, gt_joints: torch.Tensor) -> torch.Tensor:
    return compute_MPJPE(compute_similarity_transform(pred_joints, gt_joints), gt_joints)


def compute_PA_MPJPE_joints(pred_joints: torch.Tensor, gt_joints: torch.Tensor, joints_ids: List[int]) -> torch.Tensor:
    return compute_MPJPE_joints(compute_similarity_transform(pred_joints, gt_joints), gt_joints, joints_ids)


def compute_PA_MPJVE(pred_joints: torch.Tensor, gt_joints: torch.Tensor, freq: float) -> torch.Tensor:
    return _velocity_error(compute_similarity_transform(pred_joints, gt_joints), gt_joints, freq)


def compute_PA_MPJVE_joints(pred_joints: torch.Tensor, gt_joints: torch.Tensor, freq: float,
                            joints_ids: List[int]) -> torch.Tensor:
    return _velocity_error(compute_similarity_transform(pred_joints, gt_joints), gt_joints, freq, joints_ids)


def compute_V2V(pred_vertices: torch.Tensor, gt_vertices: torch.Tensor) -> torch.Tensor:
    return torch.mean(torch.norm(pred_vertices - gt_vertices, dim=-1))


def compute_similarity_transform(S1: torch.Tensor, S2: torch.Tensor) -> torch.Tensor:
    """Per-frame orthogonal Procrustes: S1 [B,N,3] mapped by the similarity (s R, t) that brings it closest to S2
    (metrics.py:141-190, the HMR2.0 formulation: R = V Z U^T from the SVD of the 3x3 cross-covariance, Z fixing
    det R = +1, s = tr(R K) / var(S1))."""
    X1 = S1.permute(0, 2, 1)
    X2 = S2.permute(0, 2, 1)
    mu1 = X1.mean(dim=2, keepdim=True)
    mu2 = X2.mean(dim=2, keepdim=True)
    X1c, X2c = X1 - mu1, X2 - mu2
    var1 = (X1c ** 2).sum(dim=(1, 2))
    K = torch.matmul(X1c, X2c.permute(0, 2, 1))
    U, _, Vh = torch.linalg.svd(K)
    V = Vh.permute(0, 2, 1)
    Z = torch.eye(3, device=S1.device, dtype=S1.dtype).unsqueeze(0).repeat(S1.shape[0], 1, 1)
    Z[:, -1, -1] *= torch.sign(torch.linalg.det(torch.matmul(U, Vh)))
    R = torch.matmul(torch.matmul(V, Z), U.permute(0, 2, 1))
    trace = torch.matmul(R, K).diagonal(offset=0, dim1=-1, dim2=-2).sum(dim=-1)
    scale = (trace / var1)[:, None, None]
    t = mu2 - scale * torch.matmul(R, mu1)
    return (scale * torch.matmul(R, X1) + t).permute(0, 2, 1)
