"""The float64 reference of the root stage's fused closure (UUO_STAGE_ROOT / UUO_STAGE_ROOT_SHARED): loss and gradient through
torch autograd on the host, written like stage_ref64.ref_part64.

    R_f   = Rz(z_f) root_f                    (z_0 for every frame in the shared packing; the product as it is)
    v_f   = SMPL(pose_body_f fixed, betas, R_f, trans_f)
    data  = w_fc sum_fm mask_fm |x_fm - v_f,nn[f,m]|^2 / sum_fm mask_fm       (0 when no marker is present)
    shape = w_rb mean_l (betas_l - o_betas_l)^2
    tvel  = w_tv mean over (F-1) 3 entries of ((trans_{t+1} - trans_t) - (mm_{t+1} - mm_t))^2,  mm_t = mean_m x_tm over ALL columns

Host only: importable and runnable without a GPU."""
import torch
import torch.nn.functional as Fn

from stage_ref64 import _d64, _float64, stages_ref


def _root_leaves64(x, F, shared):
    """the root stage's leaves [trans 3F | z F or 1 | betas 10] of the float64 x"""
    nz = 1 if shared else F
    return [t.clone().requires_grad_(True) for t in (x[:3 * F].reshape(F, 3), x[3 * F:3 * F + nz].reshape(nz, 1, 1),
                                                    x[3 * F + nz:].reshape(1, 10))]


def _root_vertices64(smpl64, pose_body, root, leaves, F, shared):
    trans, z, betas = leaves
    zf = torch.repeat_interleave(z, repeats=F, dim=0) if shared else z
    z_root = stages_ref.compute_root_orient_z(zf) @ root
    return stages_ref._smpl_repeat_betas(smpl64, pose_body, betas, z_root, trans)["vertices"]


def root_vertices64(smpl64, pose_body, root, x, shared):
    """float64 vertices [F, V, 3] of the root stage's body at x"""
    F = pose_body.shape[0]
    with _float64(), torch.no_grad():
        pose_body, root = _d64(pose_body, root)
        leaves = _root_leaves64(x.detach().cpu().double(), F, shared)
        return _root_vertices64(smpl64, pose_body, root.reshape(F, 1, 3, 3), leaves, F, shared).numpy()


def ref_root64(smpl64, cfg, markers, pose_body, o_betas, root, x, nn, shared):
    """Root stage at x = [trans 3F | z F | betas 10] (shared: [trans 3F | z 1 | betas 10]) with the assignment `nn` [F, M] of
    vertex ids held: (loss, gradient on the leaves in the packing's order)"""
    F, M_ = markers.shape[:2]
    w = cfg["stages"]["root"]["losses"]
    with _float64():
        x = x.detach().cpu().double()
        markers, pose_body, o_betas, root = _d64(markers, pose_body, o_betas, root)
        leaves = _root_leaves64(x, F, shared)
        trans, z, betas = leaves
        v = _root_vertices64(smpl64, pose_body, root.reshape(F, 1, 3, 3), leaves, F, shared)
        vn = torch.gather(v, 1, nn.cpu().long()[..., None].expand(-1, -1, 3))
        d2 = ((markers - vn) ** 2).sum(-1)
        mask = stages_ref.get_marker_mask(markers).double()
        loss = sum(t.sum() for t in leaves) * 0.0   # (every leaf has a gradient, zeros where no term reads it)
        if float(mask.sum()) > 0.0:
            loss = loss + float(w.get("full_chamfer", 0.0)) * (mask * d2).sum() / mask.sum()
        loss = loss + float(w.get("reg_betas", 0.0)) * Fn.mse_loss(betas, o_betas.reshape(1, 10))
        if F >= 2 and float(w.get("trans_vel", 0.0)) != 0.0:
            mm = markers.mean(dim=1)
            loss = loss + float(w["trans_vel"]) * Fn.mse_loss(trans[1:] - trans[:-1], mm[1:] - mm[:-1])
        loss.backward()
    return float(loss.detach()), torch.cat([t.grad.reshape(-1) for t in leaves]).numpy()
