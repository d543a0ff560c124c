"""The float64 reference of the fused stage closures: loss and gradient of the chamfer, marker and part stages through torch
autograd on the host, with every extension term the closures carry inline (joint acceleration, foot lock, floor contact, latent
offsets).  The GPU tests judge the closures against these; the terms that come as separate gradients (capsules, joint limits,
weighted prior, key points, pose acceleration, pose mixture) are in their own <term>_ref64.py and add to what is here.

Host only: importable and runnable without a GPU."""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (importable from tests/ without pytest's conftest)
    sys.path.insert(0, ROOT)
from oracle import stages_ref  # noqa: E402


@contextlib.contextmanager
def _float64():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _d64(*ts):
    return [torch.as_tensor(t).detach().cpu().double() for t in ts]


def _rho(s, sigma):
    return s * (sigma * sigma / (sigma * sigma + s)) if sigma else s


def _accel64(joints):
    F = joints.shape[0]
    if F < 3:
        return joints.sum() * 0.0
    a = joints[:-2, :24] - 2.0 * joints[1:-1, :24] + joints[2:, :24]
    return Fn.mse_loss(a, torch.zeros_like(a))


def _lock64(joints, c):
    """The foot-lock term, float64 torch: sum_t sum_s g[t, s] |v[t, s]|^2 / ((F - 1) 6)."""
    F = joints.shape[0]
    if F < 2:
        return joints.sum() * 0.0
    c = c.double()
    v = joints[1:, 10:12] - joints[:-1, 10:12]
    g = c[1:] * c[:-1]
    return (g[..., None] * v * v).sum() / ((F - 1) * 6.0)


def _floor64(z, k_left, c, h, w_pen, w_con):
    """The floor-contact term, float64 torch, on sole heights z [F, K]; the argmin is the first in list order"""
    F, K = z.shape
    pen = torch.relu(h - z)
    loss = w_pen * (pen * pen).sum() / (F * K)
    for s, zs in enumerate((z[:, :k_left], z[:, k_left:])):
        am = torch.from_numpy(np.argmin(zs.detach().numpy(), axis=1))  # numpy: the first occurrence
        flo = torch.relu(zs.gather(1, am[:, None])[:, 0] - h)
        loss = loss + w_con * (c[:, s].double() * flo * flo).sum() / (2.0 * F)
    return loss


def _skin64(tables, rot, betas, trans, vids):
    """float64 torch SMPL at the vertices `vids` [K] (synthetic.lbs_f64's arithmetic, differentiable): v_posed [F,K,3],
    T_R [F,K,3,3], T_t [F,K,3] (translation included) and the 24 world joints [F,24,3]."""
    F = rot.shape[0]
    vt = torch.from_numpy(tables.v_template).double()
    S = torch.from_numpy(tables.shapedirs).double()
    P = torch.from_numpy(tables.posedirs).double()
    Jr = torch.from_numpy(tables.J_regressor).double()
    W = torch.from_numpy(tables.lbs_weights).double()
    v_shaped = vt[None] + torch.einsum("bl,mkl->bmk", betas.expand(F, 10), S)
    J = torch.einsum("bik,ji->bjk", v_shaped, Jr)
    pf = (rot[:, 1:] - torch.eye(3, dtype=torch.float64)).reshape(F, -1)
    Pk = P.reshape(207, -1, 3)[:, vids]
    v_posed = v_shaped[:, vids] + torch.einsum("fp,pkc->fkc", pf, Pk)
    GR, Gt = [rot[:, 0]], [J[:, 0]]
    for j in range(1, 24):
        p = int(tables.parents[j])
        GR.append(GR[p] @ rot[:, j])
        Gt.append(torch.einsum("fab,fb->fa", GR[p], J[:, j] - J[:, p]) + Gt[p])
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
    At = Gt - torch.einsum("fjab,fjb->fja", GR, J)
    T_R = torch.einsum("kj,fjab->fkab", W[vids], GR)
    T_t = torch.einsum("kj,fja->fka", W[vids], At) + trans[:, None]
    return v_posed, T_R, T_t, Gt + trans[:, None]


def _chamfer_forward64(smpl64, x, root, F):
    """the chamfer stage's leaves [trans 3F | z F | betas 10 | pose 207F] of the float64 x and the model's output on them"""
    leaves = [t.clone().requires_grad_(True) for t in (x[:3 * F].reshape(F, 3), x[3 * F:4 * F].reshape(F, 1, 1),
                                                      x[4 * F:4 * F + 10].reshape(1, 10), x[4 * F + 10:].reshape(F, 23, 3, 3))]
    trans, z, betas, pose = leaves
    z_root = stages_ref.compute_root_orient_z(z) @ root
    out = stages_ref._smpl_repeat_betas(smpl64, stages_ref.normalize_rot(pose), betas, stages_ref.normalize_rot(z_root), trans)
    return leaves, out


def _marker_leaves64(x, F):
    """the marker stage's leaves [pose 207F | betas 10 | root 9F | trans 3F] of the float64 x (latent offsets, if any, follow)"""
    n0 = 219 * F + 10
    return [t.clone().requires_grad_(True) for t in (x[:207 * F].reshape(F, 23, 3, 3), x[207 * F:207 * F + 10].reshape(1, 10),
                                                    x[207 * F + 10:216 * F + 10].reshape(F, 1, 3, 3), x[216 * F + 10:n0].reshape(F, 3))]


def _marker_forward64(smpl64, x, F):
    leaves = _marker_leaves64(x, F)
    pose, betas, root, trans = leaves
    out = stages_ref._smpl_repeat_betas(smpl64, stages_ref.normalize_rot(pose), betas, stages_ref.normalize_rot(root), trans)
    return leaves, out


def _heights64(smpl64, pose, betas, root, trans, vids, z=None):
    """float64 sole heights [F, K] of the body at (pose, betas, root, trans) -- the marker stage's parameters, or with the yaw
    angles `z` the chamfer stage's (root = Rz(z) root)"""
    with _float64(), torch.no_grad():
        pose, betas, root, trans = _d64(pose, betas, root, trans)
        if z is not None:
            root = stages_ref.compute_root_orient_z(z.detach().cpu().double()) @ root
        out = stages_ref._smpl_repeat_betas(smpl64, stages_ref.normalize_rot(pose), betas, stages_ref.normalize_rot(root), trans)
        return out["vertices"][:, vids, 2].numpy()


def _stage(cfg, name, sigma):
    st = cfg["stages"][name]
    return st, st["losses"], float(st.get("robust_sigma", 0.0)) if sigma is None else sigma


def ref_chamfer64(smpl64, cfg, markers, o_pose, o_betas, root, x, nn, contacts=None, vids=None, k_left=None, sigma=None,
                  with_vertices=False):
    """Chamfer stage at x with the assignment `nn`: (loss, flat gradient), and the float64 vertices with `with_vertices`.
    `contacts` [F, 2] brings the foot-lock term in, the sole `vids` / `k_left` (with contacts) the floor term; a term whose
    evidence is absent is left out of the sum, not multiplied by zero.  `sigma` overrides the stage's robust_sigma."""
    F = markers.shape[0]
    st, w, sigma = _stage(cfg, "chamfer", sigma)
    with _float64():
        markers, o_pose, o_betas, root = _d64(markers, o_pose, o_betas, root)
        leaves, out = _chamfer_forward64(smpl64, torch.as_tensor(x).detach().cpu().double(), root, F)
        trans, z, betas, pose = leaves
        vn = torch.gather(out["vertices"], 1, torch.as_tensor(nn).cpu().long()[..., None].expand(-1, -1, 3))
        mask = stages_ref.get_marker_mask(markers).double()
        d2 = ((markers - vn) ** 2).sum(-1)
        loss = (mask * _rho(d2, sigma)).sum() / mask.sum() * w["full_chamfer"] + \
            Fn.mse_loss(pose, o_pose) * w["reg_pose_body"] + Fn.mse_loss(betas, o_betas) * w["reg_betas"] + \
            _accel64(out["joints"]) * w.get("joint_accel", 0.0)
        if contacts is not None:
            loss = loss + _lock64(out["joints"][:, :24], contacts) * w.get("foot_lock", 0.0)
        if vids is not None:
            loss = loss + _floor64(out["vertices"][:, vids, 2], k_left, contacts, float(st["floor_height"]),
                                   w.get("floor_penetration", 0.0), w.get("floor_contact", 0.0))
        loss.backward()
    res = float(loss.detach()), torch.cat([t.grad.reshape(-1) for t in leaves]).numpy()
    return res + (out["vertices"].detach().numpy(),) if with_vertices else res


def ref_marker64(smpl64, tables, cfg, markers, o_pose, o_betas, x, assign, bary=None, contacts=None, vids=None, k_left=None,
                 num_markers=None, sigma=None):
    """Marker stage at x, (loss, flat gradient): through the float64 SmplInference without the latent offsets, through _skin64
    (which has the blended rotations the offsets need; `tables` is read in this branch only) with them.  `contacts`, `vids` /
    `k_left` and `sigma` as in ref_chamfer64."""
    from uuo_mocap_amd.engine import MARKER_DISTANCE

    F = markers.shape[0]
    M = markers.shape[1] if num_markers is None else num_markers
    st, w, sigma = _stage(cfg, "marker", sigma)
    w_offs = float(w.get("latent_offsets", 0.0))
    n0 = 219 * F + 10
    with _float64():
        x = x.detach().cpu().double()
        markers, o_pose, o_betas = _d64(markers, o_pose, o_betas)
        a = torch.as_tensor(assign).cpu().long()
        mask = stages_ref.get_marker_mask(markers).double()
        if w_offs:
            leaves = _marker_leaves64(x, F)
            pose, betas, root, trans = leaves
            offs = x[n0:].reshape(M, 3).clone().requires_grad_(True)
            leaves.append(offs)
            rot = torch.cat([stages_ref.normalize_rot(root), stages_ref.normalize_rot(pose)], dim=1)
            a2 = a.reshape(M, -1)
            K = a2.shape[1]
            vp, T_R, T_t, joints = _skin64(tables, rot, betas, trans, a2.reshape(-1) if vids is None else torch.cat([a2.reshape(-1), vids]))
            nk = M * K
            pts = vp[:, :nk].reshape(F, M, K, 3) + offs[None, :, None]
            vk = torch.einsum("fmkab,fmkb->fmka", T_R[:, :nk].reshape(F, M, K, 3, 3), pts) + T_t[:, :nk].reshape(F, M, K, 3)
            b = torch.ones(M, 1) if bary is None else bary.cpu().double()
            vm = (vk * b[None, :, :, None]).sum(2)
            data = torch.mean(_rho(((markers - vm) ** 2).sum(-1), sigma) * mask)
            prior = torch.mean((offs.norm(dim=1) - MARKER_DISTANCE) ** 2) * w_offs
            if vids is not None:
                sole_z = (torch.einsum("fkab,fkb->fka", T_R[:, nk:], vp[:, nk:]) + T_t[:, nk:])[..., 2]  # (no offset on a sole point)
        else:
            leaves, out = _marker_forward64(smpl64, x, F)
            pose, betas, root, trans = leaves
            v, joints = out["vertices"], out["joints"][:, :24]
            vm = v[:, a] if bary is None else (v[:, a] * bary.cpu().double()[None, :, :, None]).sum(2)
            e = torch.norm(markers - vm, dim=-1) - MARKER_DISTANCE
            data = torch.mean(_rho(e ** 2, sigma) * mask)
            prior = 0.0
            if vids is not None:
                sole_z = v[:, vids, 2]
        loss = data * w["marker"] + Fn.mse_loss(pose, o_pose) * w["reg_pose_body"] + Fn.mse_loss(betas, o_betas) * w["reg_betas"] + \
            prior + _accel64(joints) * w.get("joint_accel", 0.0)
        if contacts is not None:
            loss = loss + _lock64(joints, contacts) * w.get("foot_lock", 0.0)
        if vids is not None:
            loss = loss + _floor64(sole_z, k_left, contacts, float(st["floor_height"]), w.get("floor_penetration", 0.0),
                                   w.get("floor_contact", 0.0))
        loss.backward()
    return float(loss.detach()), torch.cat([t.grad.reshape(-1) for t in leaves]).numpy()


def ref_part64(smpl64, cfg, markers, pose_body, o_betas, root, x, vidx, nn, sigma=0.0):
    """Part stage at x = [z 1 | trans 3F | betas 10] on the cached pose, with the assignment `nn` among the candidates `vidx`"""
    F, M_ = markers.shape[:2]
    w = cfg["stages"]["part"]["losses"]
    with _float64():
        x = x.detach().cpu().double()
        markers, pose_body, o_betas, root = _d64(markers, pose_body, o_betas, root)
        leaves = [t.clone().requires_grad_(True) for t in (x[:1].reshape(1, 1, 1), x[1:3 * F + 1].reshape(F, 3),
                                                          x[3 * F + 1:].reshape(1, 10))]
        z, trans, betas = leaves
        z_root = stages_ref.compute_root_orient_z(torch.repeat_interleave(z, repeats=F, dim=0)) @ root
        v = stages_ref._smpl_repeat_betas(smpl64, pose_body, betas, z_root, trans)["vertices"]
        vsel = vidx.cpu().long()[nn.cpu().long()]                     # candidate position -> vertex id, [F, M]
        vn = torch.gather(v, 1, vsel[..., None].expand(-1, -1, 3))
        d2 = ((markers - vn) ** 2).sum(-1)
        loss = _rho(d2, sigma).sum() / float(F * M_) * w["chamfer"] + Fn.mse_loss(betas, o_betas) * w["reg_betas"]
        loss.backward()
    return float(loss.detach()), torch.cat([t.grad.reshape(-1) for t in leaves]).numpy()
