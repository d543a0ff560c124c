"""Loss operators with the reference's signatures (reference src/video_mocap/losses/chamfer_distance.py:5-21,
losses/losses.py:43-51)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .engine import _f32, _ptr, check, current_stream


class _Knn1(torch.autograd.Function):
    """K=1 nearest neighbour on the GPU (uuo_nn_argmin).  Backward = pytorch3d's knn backward:
    g = 2*grad*(x - y[idx]); +g to x, -g scattered to y[idx]."""

    @staticmethod
    def forward(ctx, x, y):
        lib = _lib.load()
        xd, yd = _f32(x, "x"), _f32(y, "y")
        N, P1, P2 = xd.shape[0], xd.shape[1], yd.shape[1]
        dist = torch.empty((N, P1), dtype=torch.float32, device=xd.device)
        idx = torch.empty((N, P1), dtype=torch.int32, device=xd.device)
        ws = torch.empty((max(N * P1, 1),), dtype=torch.int64, device=xd.device)
        with torch.cuda.device(xd.device):
            check(lib.uuo_nn_argmin(current_stream(xd.device), N, P1, P2, _ptr(xd), _ptr(yd), None, 0, _ptr(dist),
                                    _ptr(idx), _ptr(ws)), "uuo_nn_argmin")
        idx64 = idx.long()
        ctx.save_for_backward(xd, yd, idx64)
        ctx.mark_non_differentiable(idx64)
        return dist, idx64

    @staticmethod
    def backward(ctx, grad_dist, _):
        x, y, idx = ctx.saved_tensors
        gidx = idx[..., None].expand(-1, -1, 3)
        g = 2.0 * grad_dist[..., None] * (x - torch.gather(y, 1, gidx))
        # accumulate with index_put_ (sort-based on the GPU, fixed summation order) rather than scatter_add_ (float
        # atomics): several x points may share a nearest y point, and the solves built on this operator must be
        # reproducible run to run
        rows = (torch.arange(y.shape[0], device=y.device)[:, None] * y.shape[1] + idx).reshape(-1)
        gy = torch.zeros((y.shape[0] * y.shape[1], 3), dtype=y.dtype, device=y.device)
        gy.index_put_((rows,), -g.reshape(-1, 3), accumulate=True)
        return g, gy.view_as(y)


def knn_points_k1(x: torch.Tensor, y: torch.Tensor):
    """(squared distances [N,P1], indices [N,P1] int64) of each x point's nearest y point (first index on ties)."""
    return _Knn1.apply(x, y)


def chamfer_distance(x, y, weights=None, single_directional: bool = False):
    """pytorch3d.loss.chamfer_distance with its defaults (mean/mean, squared L2), as the reference calls it at
    markers/markers_utils.py:471-475,575-579."""
    N = x.shape[0]

    def one_way(a, b):
        d, _ = knn_points_k1(a, b)
        if weights is not None:
            if weights.sum() == 0.0:
                return (a.sum((1, 2)) * weights).sum() * 0.0
            d = d * weights.view(N, 1)
        d = d.sum(1) / float(max(a.shape[1], 1))
        div = weights.sum() if weights is not None else max(N, 1)
        return d.sum() / div

    cham = one_way(x, y)
    if not single_directional:
        cham = cham + one_way(y, x)
    return cham, None


class _SoftMin(torch.autograd.Function):
    """EXTENSION (not in the reference): soft-min of the squared distances to a cloud, uuo_soft_nn_forward/backward."""

    @staticmethod
    def forward(ctx, x, y, tau):
        lib = _lib.load()
        xd, yd = _f32(x, "x"), _f32(y, "y")
        N, P1, P2 = xd.shape[0], xd.shape[1], yd.shape[1]
        soft = torch.empty((N, P1), dtype=torch.float32, device=xd.device)
        dmin = torch.empty_like(soft)
        sumexp = torch.empty_like(soft)
        ws = torch.empty((max(N * P1, 1),), dtype=torch.int64, device=xd.device)
        with torch.cuda.device(xd.device):
            check(lib.uuo_soft_nn_forward(current_stream(xd.device), N, P1, P2, _ptr(xd), _ptr(yd), float(tau), _ptr(soft),
                                          _ptr(dmin), _ptr(sumexp), _ptr(ws)), "uuo_soft_nn_forward")
        ctx.save_for_backward(xd, yd, dmin, sumexp)
        ctx.tau = float(tau)
        return soft

    @staticmethod
    def backward(ctx, grad_soft):
        x, y, dmin, sumexp = ctx.saved_tensors
        lib = _lib.load()
        g = _f32(grad_soft, "grad")
        N, P1, P2 = x.shape[0], x.shape[1], y.shape[1]
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(x.device):
            check(lib.uuo_soft_nn_backward(current_stream(x.device), N, P1, P2, _ptr(x), _ptr(y), ctx.tau, _ptr(dmin),
                                           _ptr(sumexp), _ptr(g), _ptr(gx), _ptr(gy)), "uuo_soft_nn_backward")
        return gx, gy, None


def soft_weighted_chamfer_distance(x: torch.Tensor, y: torch.Tensor, x_weights: torch.Tensor, tau: float):
    """EXTENSION, not reference behaviour: `weighted_chamfer_distance` with the hard minimum over the vertices replaced
    by the soft minimum  -tau log sum_j exp(-|x_i - y_j|^2 / tau)  (-> the hard term as tau -> 0).  Same normalisation."""
    d = _SoftMin.apply(x, y, tau)
    w = x_weights.to(d.dtype) if x_weights.dtype != d.dtype else x_weights
    wsum = x_weights.sum()
    if wsum == 0.0:
        return (x.sum() * 0.0), None
    return (d * w).sum() / wsum, None


def soft_chamfer_distance(x: torch.Tensor, y: torch.Tensor, tau: float):
    """EXTENSION, not reference behaviour: the one-directional `chamfer_distance(x, y, single_directional=True)` of the part
    stage (markers_utils.py:471-475: mean over the clouds of the mean over the points, unmasked) with the hard minimum over
    the candidate vertices replaced by the soft minimum -tau log sum_j exp(-|x_i - y_j|^2 / tau)."""
    d = _SoftMin.apply(x, y, tau)                      # [N, P1]
    return d.sum(1).div(float(max(x.shape[1], 1))).sum() / float(max(x.shape[0], 1)), None


def weighted_chamfer_distance(x: torch.Tensor, y: torch.Tensor, x_weights: torch.Tensor,
                              single_directional: bool = False):
    """sum_{n,i} w[n,i] * min_j |x[n,i]-y[n,j]|^2 / sum(w)  (the reference flattens to one cloud per marker and
    repeats y per marker -- 1.24 GB at F=300, M=50; here y is read in place).  Like the reference
    (chamfer_distance.py:19) the `single_directional` argument is ignored: always marker -> vertex."""
    d, _ = knn_points_k1(x, y)
    w = x_weights.to(d.dtype) if x_weights.dtype != d.dtype else x_weights
    wsum = x_weights.sum()
    if wsum == 0.0:
        return (x.sum() * 0.0), None
    return (d * w).sum() / wsum, None


class _RingDistance(torch.autograd.Function):
    """EXTENSION (not in the reference): distance of every x[f, m] to the one-ring of its nearest vertex (uuo_nn_argmin +
    uuo_ring_closest_points on `model`'s faces).  Backward: the barycentric weights are held fixed (exact where the distance is
    differentiable), g = grad (x - p) / r: +g to x, -b_k g scattered to the winning face's three corners; r = 0 gives none."""

    @staticmethod
    def forward(ctx, x, vertices, model):
        xd, vd = _f32(x, "x"), _f32(vertices, "vertices")
        _, nn = model.nn_argmin(xd, vd)
        dist, face, closest, bary = model.ring_closest_points(vd, xd, nn)
        nn64 = nn.long()
        corners = torch.where(face[..., None] >= 0, model.faces[face.clamp(min=0).long()], nn64[..., None].expand(-1, -1, 3))
        ctx.save_for_backward(xd, closest, dist, corners, bary)
        ctx.v_shape = vd.shape
        ctx.mark_non_differentiable(nn64, corners, bary)
        return dist, nn64, corners, bary

    @staticmethod
    def backward(ctx, grad_dist, _nn, _corners, _bary):
        x, closest, dist, corners, bary = ctx.saved_tensors
        safe = torch.where(dist > 0, dist, torch.ones_like(dist))
        g = torch.where(dist > 0, grad_dist / safe, torch.zeros_like(dist))[..., None] * (x - closest)
        F_, V_ = ctx.v_shape[0], ctx.v_shape[1]
        # index_put_ (sort-based, fixed summation order) rather than float atomics: see _Knn1.backward
        rows = (torch.arange(F_, device=x.device)[:, None, None] * V_ + corners).reshape(-1)
        gv = torch.zeros((F_ * V_, 3), dtype=x.dtype, device=x.device)
        gv.index_put_((rows,), (-bary[..., None] * g[:, :, None, :]).reshape(-1, 3), accumulate=True)
        return g, gv.view(ctx.v_shape), None


def surface_chamfer_distance(x: torch.Tensor, vertices: torch.Tensor, x_weights: torch.Tensor, smpl_inference_or_model,
                             distance: float = 0.0, sigma: float = 0.0):
    """EXTENSION, not reference behaviour: `weighted_chamfer_distance` with every marker's squared nearest-VERTEX distance
    replaced by (r - distance)^2, r its distance to the SURFACE on the one-ring of its nearest vertex (the faces incident to
    it; a vertex without a face stands for itself) and `distance` the marker's stand-off; `sigma` > 0 passes the square through
    gmof.  Same mask and normalisation.  What the fused chamfer closure computes with uuo_fit_set_surface, composed from the
    operators.  `smpl_inference_or_model`: a SmplInference or its engine.DeviceModel (the faces come from it)."""
    model = getattr(smpl_inference_or_model, "device_model", smpl_inference_or_model)
    if not getattr(model, "has_faces", False):
        raise RuntimeError("surface_chamfer_distance needs a body model with faces")
    r = _RingDistance.apply(x, vertices, model)[0]
    w = x_weights.to(r.dtype) if x_weights.dtype != r.dtype else x_weights
    wsum = x_weights.sum()
    if wsum == 0.0:
        return (x.sum() * 0.0), None
    return (gmof((r - float(distance)) ** 2, sigma) * w).sum() / wsum, None


def MarkerLoss(markers, virtual_markers, marker_weights, marker_distance):
    """[F,M] squared deviation of the marker-to-skin distance from `marker_distance`, masked."""
    gap = torch.norm(markers - virtual_markers, dim=-1) - marker_distance
    return gap ** 2 * marker_weights


def gmof(s: torch.Tensor, sigma: float) -> torch.Tensor:
    """EXTENSION, not reference behaviour: the Geman-McClure term of SMPLify's GMoF on a squared residual s (sigma in metres),
    rho(s) = s sigma^2 / (sigma^2 + s): ~ s for s << sigma^2, bounded by sigma^2.  sigma = 0 returns s unchanged (the
    reference's square).  What the fused closures apply per data item (uuo_problem_t.robust_sigma)."""
    if not sigma:
        return s
    sig2 = float(sigma) * float(sigma)
    return s * (sig2 / (sig2 + s))


def gmof_grad(s: torch.Tensor, sigma: float) -> torch.Tensor:
    """d gmof / d s = (sigma^2 / (sigma^2 + s))^2 (1 for sigma = 0)."""
    if not sigma:
        return torch.ones_like(s)
    sig2 = float(sigma) * float(sigma)
    return (sig2 / (sig2 + s)) ** 2


def robust_weighted_chamfer_distance(x: torch.Tensor, y: torch.Tensor, x_weights: torch.Tensor, sigma: float):
    """EXTENSION: `weighted_chamfer_distance` with every marker's squared nearest-vertex distance d passed through gmof."""
    d, _ = knn_points_k1(x, y)
    w = x_weights.to(d.dtype) if x_weights.dtype != d.dtype else x_weights
    wsum = x_weights.sum()
    if wsum == 0.0:
        return (x.sum() * 0.0), None
    return (gmof(d, sigma) * w).sum() / wsum, None


def robust_chamfer_distance(x: torch.Tensor, y: torch.Tensor, sigma: float):
    """EXTENSION: the part stage's one-directional `chamfer_distance(x, y, single_directional=True)` (mean over the clouds of
    the mean over the points, unmasked) with every squared nearest-vertex distance passed through gmof."""
    d, _ = knn_points_k1(x, y)                          # [N, P1]
    return gmof(d, sigma).sum(1).div(float(max(x.shape[1], 1))).sum() / float(max(x.shape[0], 1)), None


def RobustMarkerLoss(markers, virtual_markers, marker_weights, marker_distance, sigma: float):
    """EXTENSION: `MarkerLoss` with the squared deviation passed through gmof."""
    gap = torch.norm(markers - virtual_markers, dim=-1) - marker_distance
    return gmof(gap ** 2, sigma) * marker_weights


def joint_accel_loss(joints: torch.Tensor) -> torch.Tensor:
    """EXTENSION (not in the reference): the joint-acceleration smoothness term of the fused chamfer and marker closures
    (uuo_fit_set_joint_accel) on joint positions [F, J, 3] -- F.mse_loss of the second differences
    a_t = J_t - 2 J_{t+1} + J_{t+2}, t = 0 .. F-3, against zero, i.e. sum_t |a_t|^2 / ((F - 2) 3 J).  Units: m^2 per frame^2.
    With fewer than three frames there are no terms and the value is 0."""
    if joints.shape[0] < 3:
        return joints.sum() * 0.0
    a = joints[:-2] - 2.0 * joints[1:-1] + joints[2:]
    return torch.mean(a * a)


def foot_lock_loss(joints: torch.Tensor, contacts: torch.Tensor) -> torch.Tensor:
    """EXTENSION (not in the reference): the contact-gated foot-lock term of the fused chamfer and marker closures
    (uuo_fit_set_foot_lock) on joint positions [F, >= 12, 3] and contact labels [F, 2] in [0, 1] (left, right foot) --
    mean(g[..., None] * v^2) with v[t, s] = J[t, foot_s] - J[t-1, foot_s] (feet: joints 10 and 11, all three components) and
    the gate g[t, s] = c[t, s] c[t-1, s], t = 1 .. F-1, i.e. sum g |v|^2 / ((F - 1) 6).  Units: m^2 per frame^2.  With fewer
    than two frames there are no terms and the value is 0."""
    if joints.shape[0] < 2:
        return joints.sum() * 0.0
    contacts = contacts.to(device=joints.device, dtype=joints.dtype)
    v = joints[1:, 10:12] - joints[:-1, 10:12]
    g = contacts[1:] * contacts[:-1]
    return torch.mean(g[..., None] * (v * v))



def floor_loss(vertices: torch.Tensor, vids, k_left: int, contacts, height: float, w_pen: float, w_con: float) -> torch.Tensor:
    """EXTENSION (not in the reference): the floor-contact term of the fused chamfer and marker closures (uuo_fit_set_floor),
    composed -- their checker.  vertices [F, V, 3] (z up), `vids` the K sole points' vertex ids with the left foot's `k_left`
    first, contacts [F, 2] in [0, 1] (left, right; None = no contact piece), the plane at `height`:
    w_pen mean(max(h - z, 0)^2) + w_con sum_t sum_s c[t, s] max(min_{p of s} z[t, p] - h, 0)^2 / (2 F).  The foot's lowest point
    takes the whole gradient of its piece, the first in list order on exact ties."""
    vids = torch.as_tensor(vids, dtype=torch.long, device=vertices.device)
    z = vertices[:, vids, 2]
    k_left = int(k_left)
    pen = torch.relu(float(height) - z)
    loss = float(w_pen) * torch.mean(pen * pen)
    if contacts is not None and float(w_con) != 0.0:
        contacts = contacts.to(device=z.device, dtype=z.dtype)
        for s, zs in enumerate((z[:, :k_left], z[:, k_left:])):
            is_min = zs.detach() == zs.detach().min(dim=1, keepdim=True).values
            first = is_min & (torch.cumsum(is_min.to(torch.int32), dim=1) == 1)
            flo = torch.relu(torch.sum(torch.where(first, zs, torch.zeros_like(zs)), dim=1) - float(height))
            loss = loss + float(w_con) * torch.sum(contacts[:, s] * flo * flo) / (2.0 * z.shape[0])
    return loss


def capsule_closest_params(a1: torch.Tensor, b1: torch.Tensor, a2: torch.Tensor, b2: torch.Tensor):
    """EXTENSION: closest-point parameters (s, t) in [0, 1] of the segments [a1, b1] and [a2, b2] ([..., 3]) in the tensors' own
    precision -- the routine of the self-penetration term (uuo_fit_set_capsules; Ericson, Real-Time Collision Detection 5.1.9),
    branch for branch: a segment with |b - a|^2 <= 1e-12 is a point, den = A E - b^2 <= 1e-6 A E is parallel and takes s = 0."""
    d1, d2, r = b1 - a1, b2 - a2, a1 - a2
    A, E = (d1 * d1).sum(-1), (d2 * d2).sum(-1)
    f, c, b = (d2 * r).sum(-1), (d1 * r).sum(-1), (d1 * d2).sum(-1)
    dA, dE = A <= 1e-12, E <= 1e-12
    zero = torch.zeros_like(A)
    one = torch.ones_like(A)
    As, Es = torch.where(dA, one, A), torch.where(dE, one, E)  # (the degenerate branches never use the quotient)
    den = A * E - b * b
    ok = den > 1e-6 * (A * E)
    s = torch.where(ok, ((b * f - c * E) / torch.where(ok, den, one)).clamp(0.0, 1.0), zero)
    t = (b * s + f) / Es
    s = torch.where(t < 0.0, (-c / As).clamp(0.0, 1.0), torch.where(t > 1.0, ((b - c) / As).clamp(0.0, 1.0), s))
    t = t.clamp(0.0, 1.0)
    s = torch.where(dE, (-c / As).clamp(0.0, 1.0), s)
    t = torch.where(dE, zero, t)
    t = torch.where(dA, (f / Es).clamp(0.0, 1.0), t)
    s = torch.where(dA, zero, s)
    t = torch.where(dA & dE, zero, t)
    return s, t


def self_penetration_loss(joints: torch.Tensor, cap_joints, cap_geom, pairs, w: float) -> torch.Tensor:
    """EXTENSION (not in the reference): the bone-capsule self-penetration term of the fused chamfer and marker closures
    (uuo_fit_set_capsules), composed -- their checker.  joints [F, 24, 3] (the kinematic joints; the term is translation
    invariant), cap_joints [C, 2], cap_geom [C, 3] (alpha, beta, radius), pairs [P, 2]:  w sum_t sum_k max(r_i + r_j - d, 0)^2 / F
    with d the distance of the pair's segments.  The closest-point parameters are found under no_grad and held fixed (envelope
    theorem); the distance and the hinge are under autograd.  d = 0 gives no gradient, and pen^2 still counts."""
    dev = joints.device
    cj = torch.as_tensor(np.asarray(cap_joints), dtype=torch.long, device=dev).reshape(-1, 2)
    cg = torch.as_tensor(np.asarray(cap_geom), dtype=joints.dtype, device=dev).reshape(-1, 3)
    pr = torch.as_tensor(np.asarray(pairs), dtype=torch.long, device=dev).reshape(-1, 2)
    ju, jv = joints[:, cj[:, 0]], joints[:, cj[:, 1]]
    a = ju + cg[None, :, 0:1] * (jv - ju)
    b = ju + cg[None, :, 1:2] * (jv - ju)
    a1, b1, a2, b2 = a[:, pr[:, 0]], b[:, pr[:, 0]], a[:, pr[:, 1]], b[:, pr[:, 1]]
    with torch.no_grad():
        s, t = capsule_closest_params(a1, b1, a2, b2)
    delta = (a1 + s[..., None] * (b1 - a1)) - (a2 + t[..., None] * (b2 - a2))
    d2 = (delta * delta).sum(-1)
    pos = d2 > 0.0
    d = torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    pen = torch.relu(cg[pr[:, 0], 2] + cg[pr[:, 1], 2] - d)
    return float(w) * (pen * pen).sum() / joints.shape[0]


def joint_limit_loss(rot_body: torch.Tensor, lo, hi, w: float) -> torch.Tensor:
    """EXTENSION (not in the reference): the joint-angle limit term of the fused chamfer and marker closures
    (uuo_fit_set_joint_limits), composed -- their checker.  rot_body [F, 23, 3, 3] are the body joints' local rotations after the
    stage's normalisation, lo / hi [23, 3] bounds in radians on the components of each joint's axis-angle vector (-inf / +inf =
    no bound):  w sum_t sum_j sum_k (max(omega_k - hi, 0) + max(lo - omega_k, 0))^2 / F  with
    s = 1/2 (R21 - R12, R02 - R20, R10 - R01), c = 1/2 (tr R - 1), n = |s|, omega = (atan2(n, c) / n) s.  The branches are chosen
    under no_grad and in the tensors' own precision -- n < 1e-4 and c >= 0: omega = s (identity branch, kappa = 1, d kappa = 0);
    n < 1e-4 and c < 0: the joint contributes nothing (half turn) --, everything else is under autograd."""
    dev, dt = rot_body.device, rot_body.dtype
    lo = torch.as_tensor(np.asarray(lo, dtype=np.float64), dtype=dt, device=dev).reshape(23, 3)
    hi = torch.as_tensor(np.asarray(hi, dtype=np.float64), dtype=dt, device=dev).reshape(23, 3)
    R = rot_body
    s = 0.5 * torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], dim=-1)
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    n2 = (s * s).sum(-1)
    with torch.no_grad():
        small = torch.sqrt(n2) < 1e-4
        skip = small & (c < 0.0)
    one = torch.ones_like(n2)
    n = torch.sqrt(torch.where(small, one, n2))  # (the identity and half-turn branches never use the quotient)
    kappa = torch.where(small, one, torch.atan2(n, torch.where(small, one, c)) / n)
    om = kappa[..., None] * s
    pen = torch.relu(om - hi) + torch.relu(lo - om)
    pen = torch.where(skip[..., None], torch.zeros_like(pen), pen)
    return float(w) * (pen * pen).sum() / rot_body.shape[0]


def pose_gmm_loss(rot_body: torch.Tensor, means, chol, offsets, w: float, winners_out: list = None) -> torch.Tensor:
    """EXTENSION (not in the reference; SMPLify's max-mixture pose prior): the mixture pose prior of the fused chamfer and
    marker closures (uuo_fit_set_pose_gmm), composed -- their checker.  rot_body [F, 23, 3, 3] are the body joints' local
    rotations after the stage's normalisation; means [K, 69], chol [K, 69, 69] (A_k lower triangular, A_k A_k^T the inverse
    covariance) and offsets [K] are body_model.prepare_pose_mixture's:
    w sum_t min_k (1/2 |A_k^T (theta_t - mu_k)|^2 + b_k) / F,  theta the 69 axis-angle components (joint_limit_loss's omega:
    the same branches; a half turn contributes omega = 0 and receives no gradient).  The branches and the argmin (ties: the
    lowest k) are chosen under no_grad and in the tensors' own precision; everything else is under autograd, with no gradient
    through the choice.  `winners_out`, a list, receives the [F] winning components."""
    dev, dt = rot_body.device, rot_body.dtype
    mu = torch.as_tensor(np.asarray(means, dtype=np.float64), dtype=dt, device=dev).reshape(-1, 69)
    A = torch.tril(torch.as_tensor(np.asarray(chol, dtype=np.float64), dtype=dt, device=dev).reshape(-1, 69, 69))
    b = torch.as_tensor(np.asarray(offsets, dtype=np.float64), dtype=dt, device=dev).reshape(-1)
    R = rot_body
    F = R.shape[0]
    s = 0.5 * torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], dim=-1)
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    n2 = (s * s).sum(-1)
    with torch.no_grad():
        small = torch.sqrt(n2) < 1e-4
        skip = small & (c < 0.0)
    one = torch.ones_like(n2)
    n = torch.sqrt(torch.where(small, one, n2))  # (the identity and half-turn branches never use the quotient)
    kappa = torch.where(small, one, torch.atan2(n, torch.where(small, one, c)) / n)
    om = torch.where(skip[..., None], torch.zeros_like(s), kappa[..., None] * s)
    theta = om.reshape(F, 69)
    y = torch.einsum("krc,fkr->fkc", A, theta[:, None, :] - mu[None])  # A_k^T (theta - mu_k)
    e = 0.5 * (y * y).sum(-1) + b[None]
    with torch.no_grad():
        win = torch.argmin(e, dim=1)  # (the first of equal minima)
        win = torch.min(torch.where(e == e.gather(1, win[:, None]), torch.arange(e.shape[1], device=dev)[None], e.shape[1]), dim=1)[0]
        win = win.clamp(max=e.shape[1] - 1)  # (a NaN energy equals nothing)
    if winners_out is not None:
        winners_out.append(win.detach().cpu())
    return float(w) * e.gather(1, win[:, None]).sum() / F


def pose_accel_loss(rot_body: torch.Tensor, w: float, joint_weights=None) -> torch.Tensor:
    """EXTENSION (the reference's `temporal` loss on the second difference of pose_body, optimization.py:368-375, has a sign error
    and stops in a debugger): the pose-acceleration term of the chamfer and marker stages' composed closures
    (stages.<stage>.losses.pose_accel; it has no fused closure).  rot_body [F, 23, 3, 3] are the body joints' local rotations
    after the stage's normalisation, joint_weights None (ones) or 23 values >= 0 (entry j - 1 is SMPL joint j):
    w sum_t sum_j u[j] |R_t[j] - 2 R_{t+1}[j] + R_{t+2}[j]|_F^2 / ((F - 2) 207) -- with ones, w times F.mse_loss of the second
    difference against zero.  F < 3: an exact 0 that still hangs on rot_body."""
    if rot_body.shape[0] < 3:
        return rot_body.sum() * 0.0
    acc = rot_body[:-2] - 2.0 * rot_body[1:-1] + rot_body[2:]
    sq = (acc * acc).sum(dim=(-1, -2))
    if joint_weights is not None:
        u = torch.as_tensor(np.asarray(joint_weights, dtype=np.float64), dtype=rot_body.dtype, device=rot_body.device).reshape(23)
        sq = sq * u[None, :]
    return float(w) * sq.sum() / ((rot_body.shape[0] - 2) * 207.0)


def keypoints_2d_loss(joints: torch.Tensor, camera: torch.Tensor, targets: torch.Tensor, confidence: torch.Tensor, w: float,
                      sigma: float = 0.0, min_depth: float = 0.1) -> torch.Tensor:
    """EXTENSION (not in the reference, whose 2D-prior stage alone projects key points): the 2D key-point reprojection term of
    the fused chamfer and marker closures (uuo_fit_set_keypoints2d), composed -- their checker.  joints [F, >= 24, 3] (the 24
    kinematic joints count), camera [F, 16] a pinhole camera per frame in world axes (A 3x3 row-major, b, fx, fy, cx, cy),
    targets [F, 24, 2], confidence [F, 24] >= 0 (joint weights already multiplied in):
    p = A J + b,  u = (fx p_x / p_z + cx, fy p_y / p_z + cy),  s = |u - y|^2,
    w / (48 F) sum over the valid pairs of c gmof(s, sigma);  valid = c > 0 and p finite and p_z >= min_depth.
    An invalid pair contributes an exact 0 and exact zero gradient rows (it is selected away, not multiplied).  Units: the
    camera's own, squared."""
    F = joints.shape[0]
    J = joints[:, :24]
    cam = camera.to(device=J.device, dtype=J.dtype)
    y = targets.to(device=J.device, dtype=J.dtype)
    c = confidence.to(device=J.device, dtype=J.dtype)
    A, b, f, c0 = cam[:, :9].reshape(F, 3, 3), cam[:, 9:12], cam[:, 12:14], cam[:, 14:16]
    p = (A[:, None] * J[:, :, None, :]).sum(-1) + b[:, None]
    valid = (c > 0) & torch.isfinite(p).all(dim=-1) & (p[..., 2] >= float(min_depth))
    pz = torch.where(valid, p[..., 2], torch.ones_like(p[..., 2]))
    pxy = torch.where(valid[..., None], p[..., :2], torch.zeros_like(p[..., :2]))
    r = f[:, None] * pxy / pz[..., None] + c0[:, None] - y
    s = (r * r).sum(-1)
    term = torch.where(valid, c * gmof(s, sigma), torch.zeros_like(s))
    return float(w) * term.sum() / (48.0 * F)


def weighted_pose_prior(pose_body: torch.Tensor, o_pose_body: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """EXTENSION (the reference's author left it commented out, optimization.py:244): the pose prior of the fused chamfer and
    marker closures with a weight per (frame, body joint) (uuo_fit_set_prior_weights), composed -- their checker.  pose_body,
    o_pose_body [F, 23, 3, 3] raw rotations and their target, weights [F, 23] >= 0:
    sum_t sum_j w[t, j] sum_e (raw - o)^2 / (F 207) -- the mean of the weighted squares, i.e. the reference's
    weighted_mse_loss(pose_body, o_pose_body, weights[:, :, None, None]); ones give F.mse_loss.  Times reg_pose_body at the
    caller."""
    w = weights.to(device=pose_body.device, dtype=pose_body.dtype)
    d = pose_body - o_pose_body
    return torch.mean(d * d * w[:, :, None, None])
