"""The foot-lock term's parity evidence: the contact labels and the config of its parity checks (the term itself is
stage_ref64._lock64).  Host only."""
import torch

from gpu_support import W_ACCEL_C, W_ACCEL_M, W_OFFS
from uuo_mocap_amd.config import packaged_config


def _cfg(w_chamfer=0.0, w_marker=0.0, sigma=0.0, accel=False, offs=False):
    cfg = packaged_config("video_mocap")
    if w_chamfer is not None:
        cfg["stages"]["chamfer"]["losses"]["foot_lock"] = w_chamfer
    if w_marker is not None:
        cfg["stages"]["marker"]["losses"]["foot_lock"] = w_marker
    if accel:
        cfg["stages"]["chamfer"]["losses"]["joint_accel"] = W_ACCEL_C
        cfg["stages"]["marker"]["losses"]["joint_accel"] = W_ACCEL_M
    if offs:
        cfg["stages"]["marker"]["losses"]["latent_offsets"] = W_OFFS
    for k in ("chamfer", "part", "marker"):
        cfg["stages"][k]["robust_sigma"] = sigma
    return cfg


def _contacts(F, seed):
    """Random fractional labels in [0, 1] with runs of zeros (from F = 7 on; shorter sequences keep every gate open)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    c = torch.rand(F, 2, generator=gen)
    if F >= 7:
        n = max(2, F // 5)
        c[F // 3:F // 3 + n, 0] = 0.0
        c[F - n - 1:F - 1, 1] = 0.0
        c[0, 1] = 1.0
    return c
