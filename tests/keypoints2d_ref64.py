"""EXTENSION: float64 restatement of the 2D key-point reprojection term (losses.keypoints_2d_loss, uuo_fit_set_keypoints2d,
DESIGN.md section 4y) on joint positions.  The gradient comes from autograd; the closed form of the definition is restated beside
it in numpy, pair by pair, so that tests can hold the one against the other; then what the GPU parity checks of this and of later
terms share: the config keys, the float32 record and the term's gradient on the leaves of a float64 forward.  No GPU, no package
code."""
import copy

import numpy as np
import torch

from stage_ref64 import _float64

NJ = 24
MIN_DEPTH = 0.1


def gmof64(s, sigma):
    """s sigma^2 / (sigma^2 + s); sigma = 0: s"""
    if not sigma:
        return s
    s2 = float(sigma) ** 2
    return s * s2 / (s2 + s)


def project64(J, cam):
    """(p [F, 24, 3], u [F, 24, 2]) of joints J [F, 24, 3] through cam [F, 16] (A row-major, b, fx, fy, cx, cy), float64 torch;
    every component written out"""
    A, b = cam[:, :9].reshape(-1, 3, 3), cam[:, 9:12]
    p = torch.stack([A[:, None, r, 0] * J[..., 0] + A[:, None, r, 1] * J[..., 1] + A[:, None, r, 2] * J[..., 2] + b[:, None, r]
                     for r in range(3)], dim=-1)
    u = torch.stack([cam[:, None, 12] * p[..., 0] / p[..., 2] + cam[:, None, 14],
                     cam[:, None, 13] * p[..., 1] / p[..., 2] + cam[:, None, 15]], dim=-1)
    return p, u


def valid64(p, conf, min_depth):
    return (conf > 0) & torch.isfinite(p).all(dim=-1) & (p[..., 2] >= min_depth)


def keypoints2d64(J, cam, y, conf, w, sigma=0.0, min_depth=0.1):
    """w / (48 F) sum over the valid pairs of c gmof(|u - y|^2, sigma) on float64 torch joints J [F, 24, 3].  The valid pairs are
    picked by index, so that an invalid pair never enters the graph."""
    F = J.shape[0]
    with torch.no_grad():
        p0, _ = project64(J, cam)
        ok = valid64(p0, conf, min_depth)
    total = (J * 0.0).sum()
    for f, j in zip(*np.nonzero(ok.numpy())):
        _, u = project64(J[f:f + 1, j:j + 1], cam[f:f + 1])
        r = u[0, 0] - y[f, j]
        total = total + conf[f, j] * gmof64(r[0] * r[0] + r[1] * r[1], sigma)
    return float(w) * total / (48.0 * F)


def keypoints2d_grad64(J, cam, y, conf, w, sigma=0.0, min_depth=0.1):
    """(loss, d loss / d J [F, 24, 3]) by float64 autograd"""
    leaf = J.detach().double().clone().requires_grad_(True)
    loss = keypoints2d64(leaf, cam.double(), y.double(), conf.double(), w, sigma, min_depth)
    (g,) = torch.autograd.grad(loss, [leaf])
    return float(loss.detach()), g


def closed_form64(J, cam, y, conf, w, sigma=0.0, min_depth=0.1):
    """(loss, d loss / d J) of the definition in numpy float64, one pair at a time:
    k = 2 w c gmof'(s) / (48 F),  dL/dp = k (r_x fx / p_z, r_y fy / p_z, -(r_x fx p_x + r_y fy p_y) / p_z^2),  dL/dJ = A^T dL/dp"""
    J, cam, y, conf = (np.asarray(t, dtype=np.float64) for t in (J, cam, y, conf))
    F = J.shape[0]
    g, loss = np.zeros_like(J), 0.0
    for f in range(F):
        A, b, (fx, fy, cx, cy) = cam[f, :9].reshape(3, 3), cam[f, 9:12], cam[f, 12:16]
        for j in range(NJ):
            p = A @ J[f, j] + b
            c = conf[f, j]
            if not (c > 0 and np.isfinite(p).all() and p[2] >= min_depth):
                continue
            r = np.array([fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy]) - y[f, j]
            s = float(r @ r)
            q = 1.0 if not sigma else sigma ** 2 / (sigma ** 2 + s)
            loss += c * s * q
            k = 2.0 * w * c * q * q / (48.0 * F)
            dp = k * np.array([r[0] * fx / p[2], r[1] * fy / p[2], -(r[0] * fx * p[0] + r[1] * fy * p[1]) / p[2] ** 2])
            g[f, j] = A.T @ dp
    return w * loss / (48.0 * F), g


def _rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def make_camera(J, distance=4.0, focal=500.0, centre=(320.0, 240.0), swing=0.03):
    """cam [F, 16] float64 torch for z-up joints J [F, 24, 3] (numpy): a pinhole camera that looks along world +y from `distance`
    metres in front of the frame's mean joint, image x = world x, image y = -world z, turned about the vertical by `swing` rad
    per frame and with a focal length that grows 1 % per frame, so that every frame has its own row"""
    J = np.asarray(J, dtype=np.float64)
    base = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])
    rows = []
    for f in range(J.shape[0]):
        A = base @ _rz(swing * (f - 0.5 * (J.shape[0] - 1)))
        b = np.array([0.0, 0.0, distance]) - A @ J[f].mean(axis=0)
        fo = focal * (1.0 + 0.01 * f)
        rows.append(np.concatenate([A.reshape(-1), b, [fo, 1.1 * fo, centre[0], centre[1]]]))
    return torch.from_numpy(np.stack(rows))


def seeded_noise(shape, seed):
    """uniform values in [-1, 1), float64 torch, from a seeded generator"""
    gen = torch.Generator().manual_seed(int(seed))
    return 2.0 * torch.rand(*shape, generator=gen, dtype=torch.float64) - 1.0


def evidence(J, seed, noise=6.0, zero_every=7, **camera):
    """A record for joints J [F, 24, 3] (numpy float64): make_camera's rows, targets = the projection of J plus `noise` units of
    uniform noise, confidences in [0.25, 1.25) with every `zero_every`-th entry an exact 0.  float64 torch tensors."""
    cam = make_camera(J, **camera)
    _, u = project64(torch.from_numpy(np.asarray(J, dtype=np.float64)), cam)
    F = u.shape[0]
    y = u + noise * seeded_noise((F, NJ, 2), 31 + seed)
    conf = 0.75 + 0.5 * seeded_noise((F, NJ), 32 + seed)
    if zero_every:
        conf.reshape(-1)[::zero_every] = 0.0
    return {"camera": cam, "targets": y, "confidence": conf}


# ------------------------------------------------------------------------------------------------ for the GPU parity checks
def _with_key(cfg, w_chamfer, w_marker, sigma=0.0, joint_weights=None, block=True):
    cfg = copy.deepcopy(cfg)
    for stage, w in (("chamfer", w_chamfer), ("marker", w_marker)):
        cfg["stages"][stage]["losses"]["keypoints_2d"] = w
        if block:
            cfg["stages"][stage]["keypoints_2d"] = {"sigma": sigma, "min_depth": MIN_DEPTH, "joint_weights": joint_weights}
    return cfg


def _record(J, seed, **kw):
    """evidence for float64 joints J, rounded to the float32 values the device reads"""
    return {k: v.float() for k, v in evidence(np.asarray(J, dtype=np.float64), seed, **kw).items()}


def _kp_grad(leaves, out, rec, w, sigma, pad=0):
    """loss and flat gradient (numpy) of the float64 term on the leaves of a float64 forward, zero-padded by `pad` entries; the
    float64 preconditions of the issue are asserted first: every joint's depth >= 1, no confidence within 1e-4 of 0 but the
    exact zeros, no depth within 1e-4 of min_depth"""
    with _float64():
        cam, y, c = (rec[k].double() for k in ("camera", "targets", "confidence"))
        J = out["joints"][:, :24]
        p, _ = project64(J.detach(), cam)
        assert float(p[..., 2].min()) >= 1.0, "a joint nearer than 1 to the camera: pick another seed"
        assert float((p[..., 2] - MIN_DEPTH).abs().min()) >= 1e-4 and not bool(((c > 0) & (c < 1e-4)).any()), \
            "a depth within 1e-4 of min_depth or a confidence within 1e-4 of 0: pick another seed"
        assert bool((c == 0).any()) and bool((c > 0).any()), "the record needs exact-zero and positive confidences"
        loss = keypoints2d64(J, cam, y, c, w, sigma, MIN_DEPTH)
        grads = torch.autograd.grad(loss, leaves, allow_unused=True, retain_graph=True)  # (the capsules' term follows on `out`)
    g = torch.cat([(torch.zeros_like(t) if gi is None else gi).reshape(-1) for t, gi in zip(leaves, grads)]).numpy()
    return float(loss.detach()), np.concatenate([g, np.zeros(pad)])
