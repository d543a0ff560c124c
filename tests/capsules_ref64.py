"""The bone-capsule self-penetration term in float64 (the closest-point routine as plain Python per pair, distance and hinge under
torch autograd), its float64 preconditions, the capsule lists and the config of the parity checks.  Host only, so that seeds
can be checked without a GPU."""
import numpy as np
import torch

from floor_ref64 import _planes
from gpu_support import W_ACCEL_C, W_ACCEL_M, W_FLOOR_C, W_FLOOR_M, W_LOCK_C, W_LOCK_M, W_OFFS, _inputs
from stage_ref64 import _chamfer_forward64, _float64, _marker_forward64
from uuo_mocap_amd.body_model import body_capsules
from uuo_mocap_amd.config import packaged_config


# ------------------------------------------------------------------------------------------------ float64 restatement
def _clamp(v):
    return min(max(v, 0.0), 1.0)


def _closest64(a1, b1, a2, b2):
    """The issue's routine on one pair, plain float64 Python.  Returns s, t and what the preconditions look at: den / (A E)
    (None when a segment is a point or the general branch is not reached) and the unclamped parameters that were evaluated."""
    d1, d2, r = b1 - a1, b2 - a2, a1 - a2
    A, E = float(d1 @ d1), float(d2 @ d2)
    f, c, b = float(d2 @ r), float(d1 @ r), float(d1 @ d2)
    if A <= 1e-12 and E <= 1e-12:
        return 0.0, 0.0, None, []
    if A <= 1e-12:
        return 0.0, _clamp(f / E), None, [f / E]
    if E <= 1e-12:
        return _clamp(-c / A), 0.0, None, [-c / A]
    den = A * E - b * b
    raw = []
    if den > 1e-6 * A * E:
        raw.append((b * f - c * E) / den)
        s = _clamp(raw[-1])
    else:
        s = 0.0
    t = (b * s + f) / E
    raw.append(t)
    if t < 0.0:
        t = 0.0
        raw.append(-c / A)
        s = _clamp(raw[-1])
    elif t > 1.0:
        t = 1.0
        raw.append((b - c) / A)
        s = _clamp(raw[-1])
    return s, t, den / (A * E), raw


def _ends64(J, cj, cg):
    e = J[:, cj[:, 1]] - J[:, cj[:, 0]]
    return J[:, cj[:, 0]] + cg[None, :, 0:1] * e, J[:, cj[:, 0]] + cg[None, :, 1:2] * e


def _params64(J, cj, cg, pr):
    """(s, t) [F, P] and the per-pair records of _closest64 on numpy float64 joints J [F, 24, 3]"""
    a, b = _ends64(J, cj, cg)
    F, P = J.shape[0], len(pr)
    s, t, rec = np.zeros((F, P)), np.zeros((F, P)), []
    for f in range(F):
        for k, (i, j) in enumerate(pr):
            s[f, k], t[f, k], ratio, raw = _closest64(a[f, i], b[f, i], a[f, j], b[f, j])
            rec.append((f, k, ratio, raw))
    return s, t, rec


def _caps64(joints, lists, w):
    """The issue's formula, float64 torch, on joints [F, 24, 3]: the parameters from _closest64 held fixed, distance and hinge
    under autograd; pairs are summed in list order"""
    cj, cg, pr = (np.asarray(x) for x in lists)
    cg = cg.astype(np.float64)
    s, t, _ = _params64(joints.detach().numpy(), cj, cg, pr)
    cgt = torch.from_numpy(cg)
    e = joints[:, cj[:, 1]] - joints[:, cj[:, 0]]
    a = joints[:, cj[:, 0]] + cgt[None, :, 0:1] * e
    b = joints[:, cj[:, 0]] + cgt[None, :, 1:2] * e
    a1, b1, a2, b2 = a[:, pr[:, 0]], b[:, pr[:, 0]], a[:, pr[:, 1]], b[:, pr[:, 1]]
    delta = (a1 + torch.from_numpy(s)[..., None] * (b1 - a1)) - (a2 + torch.from_numpy(t)[..., None] * (b2 - a2))
    d = delta.norm(dim=-1)
    pen = torch.relu(cgt[pr[:, 0], 2] + cgt[pr[:, 1], 2] - d)
    return w * (pen * pen).sum() / joints.shape[0]


def _preconditions(J, lists, min_active):
    """The issue's float64 preconditions on joints J [F, 24, 3] (numpy) for every pair with pen > -1e-3; returns the number of
    active pairs per frame"""
    cj, cg, pr = (np.asarray(x) for x in lists)
    cg = cg.astype(np.float64)
    s, t, rec = _params64(J, cj, cg, pr)
    a, b = _ends64(J, cj, cg)
    a1, b1, a2, b2 = a[:, pr[:, 0]], b[:, pr[:, 0]], a[:, pr[:, 1]], b[:, pr[:, 1]]
    d = np.linalg.norm((a1 + s[..., None] * (b1 - a1)) - (a2 + t[..., None] * (b2 - a2)), axis=-1)
    pen = cg[pr[:, 0], 2] + cg[pr[:, 1], 2] - d
    for f, k, ratio, raw in rec:
        if pen[f, k] <= -1e-3:
            continue
        assert abs(pen[f, k]) >= 1e-4, "a pair within 1e-4 m of its hinge: pick another seed"
        assert d[f, k] >= 1e-3, "a pair's segments within 1e-3 m: pick another seed"
        assert ratio is None or ratio >= 1e-4, "a pair within 1e-4 of parallel: pick another seed"
        assert all(min(abs(v), abs(v - 1.0)) >= 1e-4 for v in raw), "a parameter within 1e-4 of a clamp: pick another seed"
    active = (pen > 0).sum(axis=1)
    assert active.min() >= min_active, "fewer than %d active pairs in a frame: pick another seed" % min_active
    return active


# ------------------------------------------------------------------------------------------------ lists and configs
def _lists(tables):
    """name -> (cap_joints, cap_geom, pairs), radii DOUBLED so that the term is active: the builder's; two capsules and one pair
    (the two thighs); the builder's cut to 65 pairs (lane 0 takes two, the others one or none); (32, 256): the builder's plus 8
    spheres (alpha == beta) along the trunk, at the hips and at the head, and 24 further pairs -- 8 sphere / sphere, 16
    sphere / segment -- most of them overlapping"""
    cj, cg, pr = body_capsules(tables)
    cg = cg.copy()
    cg[:, 2] *= 2.0
    C = len(cj)
    idx = lambda u, v: int(np.where((cj == (u, v)).all(1))[0][0])
    lt, rt = idx(1, 4), idx(2, 5)
    two = (cj[[lt, rt]], cg[[lt, rt]], np.array([[0, 1]], dtype=np.int32))
    sph_j = np.array([[9, 12], [13, 16], [14, 17], [12, 15], [1, 4], [2, 5], [0, 3], [15, 12]], dtype=np.int32)
    sph_g = np.array([[0.0, 0.0, 0.10], [0.0, 0.0, 0.10], [0.0, 0.0, 0.10], [0.0, 0.0, 0.08], [0.0, 0.0, 0.10], [0.0, 0.0, 0.10],
                      [0.5, 0.5, 0.12], [0.0, 0.0, 0.10]], dtype=np.float32)
    S = [C + k for k in range(8)]
    extra = [(S[0], S[1]), (S[0], S[2]), (S[1], S[2]), (S[4], S[5]), (S[3], S[7]), (S[6], S[4]), (S[6], S[5]), (S[0], S[3]),
             (S[4], rt), (S[5], lt), (S[1], idx(12, 15)), (S[2], idx(12, 15)), (S[0], idx(13, 16)), (S[0], idx(14, 17)),
             (S[6], lt), (S[6], rt), (S[7], idx(13, 16)), (S[7], idx(14, 17)), (S[3], idx(16, 18)), (S[3], idx(17, 19)),
             (S[1], idx(3, 6)), (S[2], idx(3, 6)), (S[4], idx(3, 6)), (S[5], idx(3, 6))]
    assert C == 24 and len(pr) == 232 and len(extra) == 24, "the builder's capsule list is not the 24 x 232 these lists extend"
    full = (np.concatenate([cj, sph_j]), np.concatenate([cg, sph_g]), np.concatenate([pr, np.array(extra, dtype=np.int32)]))
    return {"builder": (cj, cg, pr), "two": two, "cut65": (cj, cg, pr[:65]), "full": full}


def _block(lists):
    cj, cg, pr = lists
    return {"joints": [[int(v) for v in r] for r in cj], "geom": [[float(v) for v in r] for r in cg],
            "pairs": [[int(v) for v in r] for r in pr]}


def _cfg(lists=None, w_chamfer=0.0, w_marker=0.0, sigma=0.0, temporal=False, floor=None, offs=False, keys=True):
    """video_mocap.yaml with the term's keys (weight 0 = off), and the other settings of the parity checks; the floor's keys
    are always there (the stage reference reads floor_height), its weights only with `floor` = (h_chamfer, h_marker)"""
    cfg = packaged_config("video_mocap")
    for i, (stage, w, wa, wl, wf) in enumerate((("chamfer", w_chamfer, W_ACCEL_C, W_LOCK_C, W_FLOOR_C),
                                                ("marker", w_marker, W_ACCEL_M, W_LOCK_M, W_FLOOR_M))):
        st = cfg["stages"][stage]
        if keys:
            st["losses"]["self_penetration"] = w
            st["capsules"] = None if lists is None else _block(lists)
        st["floor_height"] = 0.0 if floor is None else floor[i]
        st["floor_points"] = None
        if floor is not None:
            st["losses"]["floor_penetration"] = wf
            st["losses"]["floor_contact"] = wf
        if temporal:
            st["losses"]["joint_accel"] = wa
            st["losses"]["foot_lock"] = wl
    if offs:
        cfg["stages"]["marker"]["losses"]["latent_offsets"] = W_OFFS
    for k in ("chamfer", "part", "marker"):
        cfg["stages"][k]["robust_sigma"] = sigma
    return cfg


def _joints64(smpl64, tables, F, M, seed):
    """float64 kinematic joints [F, 24, 3] (numpy) of the evaluated point of the parity case, for the chamfer closure (root =
    Rz(z) root) and for the marker closures, in the problems' packings: host only, so that seeds can be checked without a GPU"""
    _, _, _, _, root, _, (tp, zp, bp, pp, rp) = _inputs(tables, F, seed, num_markers=M)
    with _float64(), torch.no_grad():
        xc = torch.cat([tp.reshape(-1), zp.reshape(-1), bp.reshape(-1), pp.reshape(-1)]).double()
        xm = torch.cat([pp.reshape(-1), bp.reshape(-1), rp.reshape(-1), tp.reshape(-1)]).double()
        _, oc = _chamfer_forward64(smpl64, xc, root.double(), F)
        _, om = _marker_forward64(smpl64, xm, F)
        return oc["joints"][:, :24].numpy(), om["joints"][:, :24].numpy()


def _check_seed(smpl64, tables, F, M, seed):
    """every float64 precondition of the parity case (F, M, seed): the capsule lists' and the floor planes'"""
    jc, jm = _joints64(smpl64, tables, F, M, seed)
    for name, lists in _lists(tables).items():
        for J in (jc, jm):
            _preconditions(J, lists, 3 if name == "builder" else 1)
    return _planes(smpl64, tables, F, M, 6, seed)


def _caps_grad(leaves, out, lists, w, pad=0):
    """loss and flat gradient (numpy) of the float64 term on the leaves of a float64 forward, zero-padded by `pad` entries"""
    with _float64():
        loss = _caps64(out["joints"][:, :24], lists, w)
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    g = torch.cat([(torch.zeros_like(t) if gi is None else gi).reshape(-1) for t, gi in zip(leaves, grads)]).numpy()
    return float(loss.detach()), np.concatenate([g, np.zeros(pad)])
