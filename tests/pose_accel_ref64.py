"""EXTENSION: float64 torch restatement of the pose-acceleration term (losses.pose_accel_loss) on the RAW body
pose entries, with Gram-Schmidt as the chamfer and marker stages apply it.  The gradient comes from autograd; the closed-form
stencil of the definition is restated beside it, so that tests can hold the one against the other.  No GPU, no package code."""
import numpy as np
import torch


def gram_schmidt64(raw):
    """rotation_6d_to_matrix(matrix_to_rotation_6d(raw)) in the tensor's precision: rows 0 and 1 orthonormalised (F.normalize's
    eps 1e-12), row 2 their cross product.  raw [..., 3, 3]."""
    a1, a2 = raw[..., 0, :], raw[..., 1, :]
    b1 = a1 / a1.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    u2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = u2 / u2.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack([b1, b2, b3], dim=-2)


def _weights(u, like):
    if u is None:
        return torch.ones(23, dtype=like.dtype)
    return torch.as_tensor(np.asarray(u, dtype=np.float64), dtype=like.dtype).reshape(23)


def pose_accel_of_rotations64(R, w, u=None):
    """w sum_t sum_j u[j] |R_t[j] - 2 R_{t+1}[j] + R_{t+2}[j]|_F^2 / ((F - 2) 207) on local rotations R [F, 23, 3, 3]; F < 3: an
    exact 0 (attached to R, so that autograd returns zeros)"""
    F = R.shape[0]
    if F < 3:
        return (R * 0.0).sum()
    a = R[:-2] - 2.0 * R[1:-1] + R[2:]
    return float(w) * ((a * a).sum(dim=(-1, -2)) * _weights(u, R)[None, :]).sum() / ((F - 2) * 207.0)


def pose_accel64(raw, w, u=None, normalise=True):
    """the term on raw entries [F, 23, 3, 3] (float64 torch): Gram-Schmidt first when the stage normalises"""
    return pose_accel_of_rotations64(gram_schmidt64(raw) if normalise else raw, w, u)


def pose_accel_grad64(raw, w, u=None, normalise=True):
    """(loss, d loss / d raw [F, 23, 3, 3]) by float64 autograd"""
    leaf = raw.detach().double().clone().requires_grad_(True)
    loss = pose_accel64(leaf, w, u, normalise)
    (g,) = torch.autograd.grad(loss, [leaf])
    return float(loss.detach()), g


def stencil64(R, w, u=None):
    """the closed form of d loss / d R: (2 w u[j] / ((F - 2) 207)) (a_s - 2 a_{s-1} + a_{s-2}), a_t outside 0 .. F-3
    counting as 0; loops over frames"""
    R = R.detach().double()
    F = R.shape[0]
    out = torch.zeros_like(R)
    if F < 3:
        return out
    uu = _weights(u, R)
    a = [R[t] - 2.0 * R[t + 1] + R[t + 2] for t in range(F - 2)]
    zero = torch.zeros_like(R[0])
    at = lambda t: a[t] if 0 <= t <= F - 3 else zero
    for s in range(F):
        out[s] = (2.0 * float(w) / ((F - 2) * 207.0)) * uu[:, None, None] * (at(s) - 2.0 * at(s - 1) + at(s - 2))
    return out


def random_raw(F, seed, max_angle=3.0, noise=0.05):
    """raw body pose entries [F, 23, 3, 3] (float32): rotations about hashed axes by angles up to `max_angle` rad plus `noise`
    randn on every entry, so that the rows are neither unit nor orthogonal and the Gram-Schmidt backward has work to do"""
    gen = torch.Generator().manual_seed(seed)
    axis = torch.randn(F, 23, 3, generator=gen, dtype=torch.float64)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    ang = max_angle * torch.rand(F, 23, 1, generator=gen, dtype=torch.float64)
    K = torch.zeros(F, 23, 3, 3, dtype=torch.float64)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -axis[..., 2], axis[..., 1], axis[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -axis[..., 0], -axis[..., 1], axis[..., 0]
    s, c = torch.sin(ang)[..., None], torch.cos(ang)[..., None]
    R = torch.eye(3, dtype=torch.float64) + s * K + (1.0 - c) * (K @ K)
    return (R + noise * torch.randn(F, 23, 3, 3, generator=gen, dtype=torch.float64)).float()
