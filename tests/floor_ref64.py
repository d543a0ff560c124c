"""The floor-contact term's parity evidence: the sole points, the contact labels and the planes of a parity case, with the
float64 preconditions on a plane (the term itself is stage_ref64._floor64).  Host only, so that seeds can be checked without a
GPU."""
import numpy as np
import torch

from gpu_support import _inputs
from stage_ref64 import _heights64
from uuo_mocap_amd.body_model import sole_vertices

KINK = 1e-4                        # metres every sole height keeps from the plane, and a foot's two lowest points from each other


def _vids(tables, K):
    return torch.from_numpy(sole_vertices(tables, per_foot=K // 2).reshape(-1).copy()).long()


def _contacts(F, seed):
    """Hashed labels in [0, 1] with some exact 0s and 1s"""
    gen = torch.Generator().manual_seed(2000 + seed)
    c = torch.rand(F, 2, generator=gen)
    c[0, 0] = 1.0
    if F >= 3:
        c[1, 1] = 0.0
        c[F - 1, 1] = 1.0
    if F >= 7:
        n = max(2, F // 5)
        c[F // 3:F // 3 + n, 0] = 0.0
    return c


def _plane(z, k_left, c):
    """The plane of a parity case from the float64 sole heights z [F, K]: the midpoint of the widest gap of the sorted heights
    between their 30th and 70th percentile.  Asserts (float64, before anything is compared) that every height keeps KINK from
    the plane and every foot's two lowest points KINK from each other, and that both pieces of the term are active."""
    s = np.sort(z.reshape(-1))
    n = len(s)
    lo, hi = int(np.floor(0.3 * (n - 1))), int(np.ceil(0.7 * (n - 1)))
    gaps = np.diff(s[lo:hi + 1])
    i = int(np.argmax(gaps))
    h = 0.5 * (s[lo + i] + s[lo + i + 1])
    assert np.abs(z - h).min() >= KINK, "a sole height within 1e-4 m of the plane: pick another seed"
    for zs in (z[:, :k_left], z[:, k_left:]):
        if zs.shape[1] >= 2:
            two = np.sort(zs, axis=1)[:, :2]
            assert (two[:, 1] - two[:, 0]).min() >= KINK, "a foot's two lowest points within 1e-4 m: pick another seed"
    low = np.stack([z[:, :k_left].min(axis=1), z[:, k_left:].min(axis=1)], axis=1)
    assert (z < h).any() and ((low > h) & (c.numpy() > 0)).any(), "the term is not active"
    return float(h)


def _planes(smpl64, tables, F, M, K, seed):
    """(chamfer plane, marker plane) of the parity case (F, M, K, seed): host only, so that seeds can be checked without a GPU"""
    _, _, _, _, root, _, (tp, zp, bp, pp, rp) = _inputs(tables, F, seed, num_markers=M)
    contacts, vids = _contacts(F, seed), _vids(tables, K)
    return (_plane(_heights64(smpl64, pp, bp, root, tp, vids, z=zp), K // 2, contacts),
            _plane(_heights64(smpl64, pp, bp, rp, tp, vids), K // 2, contacts))
