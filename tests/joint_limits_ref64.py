"""The joint-angle limit term in float64 (the logarithm as loops per joint, the branches held fixed under torch autograd), its
float64 preconditions, the limit tables, the config, shapes, seeds and settings of the parity checks.  Host only, so that seeds
can be checked without a GPU."""
import math

import numpy as np
import torch

from capsules_ref64 import _cfg as _caps_cfg, _check_seed as _caps_check_seed
from gpu_support import W_CAPS_C, W_CAPS_M, _inputs
from oracle import stages_ref
from stage_ref64 import _float64
from uuo_mocap_amd.body_model import smpl_joint_limits

INF = float("inf")


# ------------------------------------------------------------------------------------------------ float64 restatement
def _log64(R):
    """The issue's logarithm on rotations R [F, 23, 3, 3] (numpy float64), loops: omega, theta, and the branch per joint"""
    F = R.shape[0]
    om, theta, branch = np.zeros((F, 23, 3)), np.zeros((F, 23)), np.empty((F, 23), dtype=object)
    for f in range(F):
        for j in range(23):
            r = R[f, j]
            s = 0.5 * np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
            c = 0.5 * (r[0, 0] + r[1, 1] + r[2, 2] - 1.0)
            n = math.sqrt(float(s @ s))
            theta[f, j] = math.atan2(n, c)
            if n < 1e-4:
                branch[f, j] = "identity" if c >= 0.0 else "half turn"
                om[f, j] = s if c >= 0.0 else 0.0
            else:
                branch[f, j] = "generic"
                om[f, j] = (theta[f, j] / n) * s
    return om, theta, branch


def _limits64(pose, lo, hi, w):
    """The issue's formula in float64 torch on the raw pose leaf [F, 23, 3, 3]: the stage's normalisation, then the branches of
    _log64 held fixed, everything else under autograd"""
    R = stages_ref.normalize_rot(pose)
    _, _, branch = _log64(R.detach().numpy())
    s = 0.5 * torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], dim=-1)
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    generic = torch.from_numpy(branch == "generic")
    skip = torch.from_numpy(branch == "half turn")
    n = torch.sqrt(torch.where(generic, (s * s).sum(-1), torch.ones_like(c)))
    kappa = torch.where(generic, torch.atan2(n, torch.where(generic, c, torch.ones_like(c))) / n, torch.ones_like(c))
    om = kappa[..., None] * s
    lo_t, hi_t = torch.from_numpy(np.asarray(lo, dtype=np.float64)), torch.from_numpy(np.asarray(hi, dtype=np.float64))
    pen = torch.relu(om - hi_t) + torch.relu(lo_t - om)
    pen = torch.where(skip[..., None], torch.zeros_like(pen), pen)
    return w * (pen * pen).sum() / pose.shape[0]


def _preconditions(pose, lo, hi, min_active, min_worst=0.0):
    """The issue's float64 preconditions on the raw pose [F, 23, 3, 3] (torch, any precision) before anything is compared;
    returns the number of active components per frame"""
    with _float64():
        R = stages_ref.normalize_rot(pose.detach().cpu().double()).numpy()
    om, theta, branch = _log64(R)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    assert (branch == "generic").all(), "a joint under the 1e-4 threshold: pick another seed"
    for signed in (om - hi, lo - om):   # the two hinges
        near = signed > -1e-3
        assert (np.abs(signed[near]) >= 1e-4).all(), "a component within 1e-4 rad of its hinge: pick another seed"
    active = ((om - hi) > 0) | ((lo - om) > 0)
    th = theta[active.any(-1)]
    assert ((th >= 0.05) & (th <= 2.9)).all(), "an active joint's angle outside [0.05, 2.9]: pick another seed"
    per_frame = active.reshape(active.shape[0], -1).sum(axis=1)
    assert per_frame.min() >= min_active, "fewer than %d active components in a frame: pick another seed" % min_active
    worst = np.maximum(om - hi, lo - om).max()
    assert worst >= min_worst, "no violation of %.2f rad: pick another seed" % min_worst
    return per_frame


# ------------------------------------------------------------------------------------------------ tables and configs
def _tables():
    """name -> (lo, hi) float32 [23, 3]: the builder's; every component bounded on both sides at +-0.2 rad; a mixed one-sided
    table (x from below at -0.1 on even rows, y from above at 0.1 on odd rows, z two-sided on every third row, the rest open)"""
    lo, hi = smpl_joint_limits()
    full = (np.full((23, 3), -0.2, dtype=np.float32), np.full((23, 3), 0.2, dtype=np.float32))
    mlo, mhi = np.full((23, 3), -INF, dtype=np.float32), np.full((23, 3), INF, dtype=np.float32)
    mlo[0::2, 0] = -0.1
    mhi[1::2, 1] = 0.1
    mlo[0::3, 2], mhi[0::3, 2] = -0.15, 0.25
    return {"builder": (lo, hi), "full": full, "mixed": (mlo, mhi)}


MIN_ACTIVE = {"builder": 1, "full": 3, "mixed": 1}


def _block(tab):
    return {"lo": [[float(v) for v in r] for r in tab[0]], "hi": [[float(v) for v in r] for r in tab[1]]}


def _cfg(tab=None, w_chamfer=0.0, w_marker=0.0, sigma=0.0, temporal=False, floor=None, caps=None, offs=False, keys=True):
    """capsules_ref64's config (video_mocap.yaml with the other settings of the parity checks; `caps` = a capsule list switches
    the self-penetration term on) with the term's keys (weight 0 = off)"""
    cfg = _caps_cfg(caps, W_CAPS_C if caps is not None else 0.0, W_CAPS_M if caps is not None else 0.0, sigma=sigma,
                    temporal=temporal, floor=floor, offs=offs, keys=caps is not None)
    if keys:
        for stage, w in (("chamfer", w_chamfer), ("marker", w_marker)):
            cfg["stages"][stage]["losses"]["joint_limits"] = w
            cfg["stages"][stage]["joint_limits"] = None if tab is None else _block(tab)
    return cfg


def _check_seed(smpl64, tables, F, M, seed):
    """every float64 precondition of the parity case (F, M, seed), host only: the three tables' on the evaluated pose, and
    capsules_ref64's (capsule lists and floor planes; returns the planes)"""
    pp = _inputs(tables, F, seed, num_markers=M)[6][3]
    for name, (lo, hi) in _tables().items():
        _preconditions(pp, lo, hi, MIN_ACTIVE[name], 0.05 if name == "builder" else 0.0)
    return _caps_check_seed(smpl64, tables, F, M, seed)


# the parity shapes: F in {1, 3, 7} x M in {10, 11, 50} (odd F: the last k_limit_fwd block, two frames a block, has its upper
# half idle), and F = 4 (both halves of every block at work)
SHAPES = [(F, M) for F in (1, 3, 7) for M in (10, 11, 50)] + [(4, 11)]
# seeds of the parity cases, chosen on the host: the first of 600 + 37 F + M + 1000 n (n = 0, 1, ...) that meets _check_seed
# (n > 0 mostly because the builder's table, four components, has no active one in some frame; twice a component within 1e-4 rad
# of its hinge, once a capsule pair within 1e-4 m of its, twice no violation of 0.05 rad)
SEEDS = {(1, 10): 4647, (1, 11): 1648, (3, 10): 1721, (3, 11): 1722, (7, 10): 7869, (7, 11): 7870, (7, 50): 9909}


def _seed(F, M):
    return SEEDS.get((F, M), 600 + 37 * F + M)


def _lim_grad(leaves, pose_index, tab, w, pad=0):
    """loss and flat gradient (numpy) of the float64 term on the leaves of a float64 forward, zero-padded by `pad` entries"""
    with _float64():
        loss = _limits64(leaves[pose_index], tab[0], tab[1], w)
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    g = torch.cat([(torch.zeros_like(t) if gi is None else gi).reshape(-1) for t, gi in zip(leaves, grads)]).numpy()
    return float(loss.detach()), np.concatenate([g, np.zeros(pad)])


# settings toggled off and on: (sigma, joint_accel + foot_lock, the floor term, the capsules, latent_offsets)
SETTINGS = [(0.0, False, False, False, False), (0.05, True, False, False, False), (0.0, False, True, True, True),
            (0.05, True, True, True, True)]
