"""EXTENSION: the point-to-surface chamfer term (stages.chamfer.losses.surface_chamfer, uuo_fit_set_surface) on the MI355X --
the one-ring pick against a float64 restatement, the fused closure against float64 autograd, determinism, the composed route,
the term switched off, the refusals, and what video_mocap_surface.yaml does to a fit."""
import copy
import ctypes
import dataclasses
import math
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

from oracle import stages_ref  # noqa: E402
from foot_lock_ref64 import _contacts  # noqa: E402
from gpu_support import _inputs, _rel_err, dev, smpl, smpl64  # noqa: E402,F401
from stage_ref64 import _accel64, _d64, _float64, _lock64, _rho  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

D0 = 0.0095        # MARKER_DISTANCE
# Temporal weights of the parity checks: a tenth of test_gpu_temporal's / test_gpu_foot_lock's chamfer-stage weights (10, 100).
# Those were sized so that each temporal term's gradient equals the PLAIN square's at these inputs; here the term under test is
# the data term, whose robust form (sigma 0.1 m against residuals of the same order) has a gradient several times smaller, and
# the check that it matters (more than 1e-2 of the gradient) needs the three terms comparable, not the temporal ones dominant.
W_ACCEL, W_LOCK = 1.0, 10.0


# ------------------------------------------------------------------------------------------------ float64 restatement
def _closest64(p, a, b, c):
    """Closest point of p on triangle (a, b, c), float64 numpy: (point, "cramer" barycentric weights, distance).  The region
    test of Ericson, Real-Time Collision Detection 5.1.5; a triangle without area that is a single point (a = b = c, the
    one-ring's stand-in for a vertex without a face) gives that point with weights (1, 0, 0)."""
    p, a, b, c = (np.asarray(t, np.float64) for t in (p, a, b, c))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = ab @ ap, ac @ ap
    bp, cp = p - b, p - c
    d3, d4, d5, d6 = ab @ bp, ac @ bp, ab @ cp, ac @ cp
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    if d1 <= 0 and d2 <= 0:
        v, w = 0.0, 0.0
    elif d3 >= 0 and d4 <= d3:
        v, w = 1.0, 0.0
    elif vc <= 0 and d1 >= 0 and d3 <= 0:
        v, w = d1 / (d1 - d3), 0.0
    elif d6 >= 0 and d5 <= d6:
        v, w = 0.0, 1.0
    elif vb <= 0 and d2 >= 0 and d6 <= 0:
        v, w = 0.0, d2 / (d2 - d6)
    elif va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0:
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v = 1.0 - w
    else:
        den = 1.0 / (va + vb + vc)
        v, w = vb * den, vc * den
    q = a + ab * v + ac * w
    if not (np.any(ab != 0) or np.any(ac != 0)):
        return q, np.array([1.0, 0.0, 0.0]), float(np.linalg.norm(p - q))
    wv = q - a                                           # trimesh.triangles.points_to_barycentric(method="cramer")
    d00, d01, d02, d11, d12 = ab @ ab, ab @ ac, ab @ wv, ac @ ac, ac @ wv
    inv = 1.0 / (d00 * d11 - d01 * d01)
    b2, b1 = (d00 * d12 - d01 * d02) * inv, (d11 * d02 - d01 * d12) * inv
    return q, np.array([1.0 - b1 - b2, b1, b2]), float(np.linalg.norm(p - q))


@pytest.fixture(scope="module")
def ring(tables):
    """(faces [NF, 3], the faces incident to every vertex in ascending id) by brute force."""
    faces = np.asarray(tables.faces).astype(np.int64)
    rows = [[] for _ in range(int(tables.v_template.shape[0]))]
    for t, tri in enumerate(faces.tolist()):
        for v in dict.fromkeys(tri):
            rows[v].append(t)
    return faces, rows


@pytest.fixture(scope="module")
def posed_body(smpl, tables, dev):
    """Three frames of a posed synthetic body (fp32 vertices on the device, float64 copy on the host): computed once."""
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, 3, 411)
    from uuo_mocap_amd.transforms import normalize_rot

    with torch.no_grad():
        out = smpl(poses=normalize_rot(pp.to(dev)), betas=bp.to(dev).repeat(3, 1), root_orient=normalize_rot(rp.to(dev)),
                   trans=tp.to(dev))
    v = out["vertices"].detach().float().contiguous()
    return v, v.cpu().double().numpy()


# ------------------------------------------------------------------------------------------------ 1. the pick operator
@pytest.mark.parametrize("M", [1, 15, 16, 17, 65])
@pytest.mark.parametrize("F", [1, 3])
def test_ring_pick_operator_against_float64(smpl, posed_body, ring, dev, F, M):
    """uuo_nn_argmin + uuo_ring_closest_points on a posed body against the float64 restatement over the same one-ring.
    Face ids are not compared (a near-tie may flip); the float64 distance AT the GPU's face must be within `slack` of the
    float64 minimum over the ring, and closest point and weights must be float64's at that face.
    slack: the operator's inputs are exact in both precisions; from them to a candidate's distance the kernel does about 20
    rounded fp32 operations (differences, six dot products, a quotient, the point a + v ab + w ac, the norm), each off by at
    most 2^-24 relative to a quantity no larger than the scene's largest coordinate `scale`, so a candidate's distance is off by
    at most 20 x 2^-24 x scale and two candidates can swap order when they differ by twice that: 64 x 2^-24 x scale (7.6 um at
    2 m) covers it with the closest point's own error.  A weight moves by (closest-point error) / (the face's smallest height)."""
    faces, rows = ring
    verts_d, verts64 = posed_body
    verts_d, verts64 = verts_d[:F].contiguous(), verts64[:F]
    V = verts64.shape[1]
    valence = np.array([len(r) for r in rows])
    gen = np.random.default_rng(1000 * F + M)
    pts = np.zeros((F, M, 3), np.float32)
    base = gen.integers(0, V, size=(F, M))
    dirs = gen.standard_normal((F, M, 3))
    pts[:] = (verts64[np.arange(F)[:, None], base] + D0 * dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)
    v_none, v_nine = int(np.flatnonzero(valence == 0)[0]), int(np.flatnonzero(valence == 9)[0])
    mid = None  # an edge whose midpoint has one of the edge's ends as its nearest vertex (so the edge is in the ring searched)
    for t_edge in range(2000, 2100):
        i, j = int(faces[t_edge, 0]), int(faces[t_edge, 1])
        mid = (0.5 * (verts64[0, i] + verts64[0, j])).astype(np.float32)
        if int(np.argmin(np.linalg.norm(verts64[0] - mid.astype(np.float64), axis=1))) in (i, j):
            break
    else:
        raise AssertionError("no usable edge among faces 2000..2099")
    specials = {
        "on a vertex": verts64[0, 1234].astype(np.float32),
        "edge midpoint": mid,
        "face-less vertex": (verts64[0, v_none] + np.array([0.0, 0.0, 1e-4])).astype(np.float32),
        "valence 9": (verts64[0, v_nine] + np.array([0.0, 2e-3, 0.0])).astype(np.float32),
        "hidden": np.zeros(3, np.float32),
    }
    names = list(specials)
    placed = {}
    if M >= len(names):
        for k, n in enumerate(names):
            pts[0, k], placed[n] = specials[n], k
    else:  # a single query: another special per case
        n = names[(F + M) % len(names)]
        pts[0, 0], placed[n] = specials[n], 0
    model = smpl.device_model
    pd = torch.from_numpy(pts).to(dev)
    _, nn = model.nn_argmin(pd, verts_d)
    dist, face, closest, bary = (t.cpu().numpy() for t in model.ring_closest_points(verts_d, pd, nn))
    nn = nn.cpu().numpy()
    scale = max(float(np.abs(verts64).max()), float(np.abs(pts).max()))
    slack = 64.0 * 2.0 ** -24 * scale
    worst = {"excess": 0.0, "closest": 0.0, "dist": 0.0, "bary": 0.0}
    for f in range(F):
        for m in range(M):
            v, p = int(nn[f, m]), pts[f, m].astype(np.float64)
            tag = (f, m, [n for n, k in placed.items() if f == 0 and k == m])
            tri = lambda t: (verts64[f, faces[t, 0]], verts64[f, faces[t, 1]], verts64[f, faces[t, 2]])
            if not rows[v]:
                assert face[f, m] == -1, tag
                q, b, d = _closest64(p, verts64[f, v], verts64[f, v], verts64[f, v])
                np.testing.assert_array_equal(bary[f, m], [1.0, 0.0, 0.0], err_msg=str(tag))
                np.testing.assert_array_equal(closest[f, m], verts64[f, v].astype(np.float32), err_msg=str(tag))
                h_min = 1.0
            else:
                t = int(face[f, m])
                assert t in rows[v], tag
                d_min = min(_closest64(p, *tri(r))[2] for r in rows[v])
                q, b, d = _closest64(p, *tri(t))
                worst["excess"] = max(worst["excess"], d - d_min)
                assert d <= d_min + slack, (tag, d, d_min)
                a_, b_, c_ = tri(t)
                area2 = np.linalg.norm(np.cross(b_ - a_, c_ - a_))
                h_min = area2 / max(np.linalg.norm(b_ - a_), np.linalg.norm(c_ - a_), np.linalg.norm(c_ - b_))
            worst["closest"] = max(worst["closest"], float(np.abs(closest[f, m] - q).max()))
            worst["dist"] = max(worst["dist"], abs(float(dist[f, m]) - d))
            worst["bary"] = max(worst["bary"], float(np.abs(bary[f, m] - b).max() * h_min))
            np.testing.assert_allclose(closest[f, m], q, rtol=0, atol=slack, err_msg=str(tag))
            np.testing.assert_allclose(dist[f, m], d, rtol=0, atol=slack, err_msg=str(tag))
            np.testing.assert_allclose(bary[f, m], b, rtol=0, atol=slack / h_min, err_msg=str(tag))
    if "face-less vertex" in placed:
        assert nn[0, placed["face-less vertex"]] == v_none and face[0, placed["face-less vertex"]] == -1
    if "valence 9" in placed:
        assert nn[0, placed["valence 9"]] == v_nine
    if "on a vertex" in placed:
        assert nn[0, placed["on a vertex"]] == 1234 and dist[0, placed["on a vertex"]] <= slack
    if "edge midpoint" in placed:
        assert dist[0, placed["edge midpoint"]] <= slack
    print("OBS ring pick F %d M %d: slack %.2e m; worst distance over the ring's minimum %.2e, closest point off %.2e, "
          "distance off %.2e, weight off x height %.2e" % (F, M, slack, worst["excess"], worst["closest"], worst["dist"],
                                                           worst["bary"]))


# ------------------------------------------------------------------------------------------------ 2. closure parity
def _cfg(d0=D0, sigma=0.0, temporal=False, w=10.0):
    cfg = packaged_config("video_mocap")
    losses = cfg["stages"]["chamfer"]["losses"]
    losses.pop("full_chamfer")
    losses["surface_chamfer"] = w
    cfg["stages"]["chamfer"]["surface_distance"] = d0
    cfg["stages"]["chamfer"]["robust_sigma"] = sigma
    if temporal:
        losses["joint_accel"], losses["foot_lock"] = W_ACCEL, W_LOCK
    return cfg


def _priors_only(cfg):
    cfg = copy.deepcopy(cfg)
    cfg["stages"]["chamfer"]["losses"].pop("surface_chamfer")
    cfg["stages"]["chamfer"]["losses"]["full_chamfer"] = 0.0
    return cfg


def _ref_surface(smpl64, cfg, markers, o_pose, o_betas, root, x, corners, contacts):
    """The issue's term in float64 autograd at the GPU's own corners: weights from the float64 closest point on the float64
    corners, held fixed; p = sum b_k v_k; s = (|x - p| - d0)^2; same mask, normaliser, priors and temporal terms."""
    F, M = markers.shape[:2]
    st = cfg["stages"]["chamfer"]
    w, sigma, d0 = st["losses"], float(st.get("robust_sigma", 0.0)), float(st["surface_distance"])
    with _float64():
        x = x.detach().cpu().double()
        markers, o_pose, o_betas, root = _d64(markers, o_pose, o_betas, root)
        leaves = [t.clone().requires_grad_(True) for t in (x[:3 * F].reshape(F, 3), x[3 * F:4 * F].reshape(F, 1, 1),
                                                          x[4 * F:4 * F + 10].reshape(1, 10), x[4 * F + 10:].reshape(F, 23, 3, 3))]
        trans, z, betas, pose = leaves
        z_root = stages_ref.compute_root_orient_z(z) @ root
        out = stages_ref._smpl_repeat_betas(smpl64, stages_ref.normalize_rot(pose), betas, stages_ref.normalize_rot(z_root),
                                            trans)
        c = corners.cpu().long()
        vk = out["vertices"][torch.arange(F)[:, None, None], c]            # [F, M, 3 corners, 3]
        vk_np, mk_np = vk.detach().numpy(), markers.numpy()
        b = np.zeros((F, M, 3))
        for f in range(F):
            for m in range(M):
                b[f, m] = _closest64(mk_np[f, m], *vk_np[f, m])[1]
        b = torch.from_numpy(b)
        p = (b[..., None] * vk).sum(2)
        r = torch.norm(markers - p, dim=-1)
        mask = stages_ref.get_marker_mask(markers).double()
        loss = (mask * _rho((r - d0) ** 2, sigma)).sum() / mask.sum() * w["surface_chamfer"] + \
            Fn.mse_loss(pose, o_pose) * w["reg_pose_body"] + Fn.mse_loss(betas, o_betas) * w["reg_betas"]
        if "joint_accel" in w:
            loss = loss + _accel64(out["joints"]) * w["joint_accel"] + _lock64(out["joints"][:, :24], contacts) * w["foot_lock"]
        loss.backward()
    return float(loss.detach()), torch.cat([t.grad.reshape(-1) for t in leaves]).numpy(), b.numpy()


def _blocks(F):
    return {"trans": slice(0, 3 * F), "z": slice(3 * F, 4 * F), "betas": slice(4 * F, 4 * F + 10), "pose": slice(4 * F + 10, None)}


@pytest.mark.parametrize("M", [1, 17, 50])
@pytest.mark.parametrize("F", [1, 2, 17])
def test_surface_closure_matches_float64_autograd(smpl, smpl64, tables, ring, dev, F, M):
    """Loss rtol 2e-5 and every gradient block below 2e-4 relative against float64 autograd at the GPU's own nearest vertices
    and corners (the bounds of the three-corner marker closure); d0 in {0, 9.5 mm}, plain and robust_sigma 0.1, without and with
    joint_accel + foot_lock.  Also: the corners are a face of the nearest vertex's one-ring, hidden markers cost nothing, two
    evaluations are bit-identical, and the term carries more than 1e-2 of the gradient."""
    from uuo_mocap_amd.engine import ChamferProblem

    faces, rows = ring
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 700 + 10 * F + M, num_markers=M)
    if M > 1:
        markers[0, 1] = 0.0                                   # a hidden marker
    contacts = _contacts(F, F)
    md = markers.to(dev)
    args = (md, o_pose.to(dev), o_betas.to(dev), root.to(dev))
    face_sets = [set(map(tuple, faces[r].tolist())) for r in rows]
    for d0 in (0.0, D0):
        for sigma in (0.0, 0.1):
            for temporal in (False, True):
                cfg = _cfg(d0, sigma, temporal)
                tag = (F, M, d0, sigma, temporal)
                prob = ChamferProblem(smpl, *args, cfg, foot_contacts=contacts)
                prob0 = ChamferProblem(smpl, *args, _priors_only(cfg), foot_contacts=contacts)
                assert prob.surface and prob.surface_distance == d0 and not prob0.surface
                x = prob.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
                loss, grad, nn = prob.evaluate(x)
                corners, bary = prob.surface_corners()
                loss2, grad2, nn2 = prob.evaluate(x)
                assert loss == loss2 and torch.equal(grad, grad2) and torch.equal(nn, nn2), tag     # no float atomics
                corners2, bary2 = prob.surface_corners()
                assert torch.equal(corners, corners2) and torch.equal(bary, bary2), tag
                _, grad0, nn0 = prob0.evaluate(x)
                assert torch.equal(nn, nn0), "d_nn_idx still reports the nearest vertex"
                cn, nnn = corners.cpu().numpy(), nn.cpu().numpy()
                mask = stages_ref.get_marker_mask(markers).numpy()
                for f in range(F):
                    for m in range(M):
                        v, tri = int(nnn[f, m]), tuple(int(i) for i in cn[f, m])
                        if not mask[f, m] or not rows[v]:
                            assert tri == (v, v, v), (tag, f, m)
                        else:
                            assert tri in face_sets[v], (tag, f, m)
                lo, g_ref, b_ref = _ref_surface(smpl64, cfg, markers, o_pose, o_betas, root, x, corners, contacts)
                g = grad.cpu().numpy()
                rel = {k: _rel_err(g[s], g_ref[s]) for k, s in _blocks(F).items()}
                share = _rel_err(g, grad0.cpu().numpy())
                b_off = float(np.abs(bary.cpu().numpy() - b_ref)[mask.astype(bool)].max()) if mask.any() else 0.0
                print("OBS surface parity %s: loss rel %.2e, gradient rel %s, weights off %.1e, term's share of the gradient %.2e"
                      % (tag, abs(loss - lo) / abs(lo), {k: "%.1e" % v for k, v in rel.items()}, b_off, share))
                np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=str(tag))
                for k, v in rel.items():
                    assert v < 2e-4, (tag, k, v)
                assert share > 1e-2, tag


# ------------------------------------------------------------------------------------------------ 3. fused vs composed
def test_fused_and_composed_surface_solves_agree(smpl, tables, dev):
    """25 L-BFGS iterations of the chamfer stage on the fused closure and on the operator-composed one (execution.surface_fused:
    False), plain and robust: the start must agree to 1e-5 and the end to 5e-2, the bounds of
    test_fused_and_composed_robust_solves_agree / ..._joint_accel_solves_agree for the chamfer pair."""
    from uuo_mocap_amd.optimization import last_stats, optim_chamfer

    F, M = 37, 50
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 21)
    md = markers.to(dev)
    first = lambda s: s.get("first_loss", s.get("loss_first"))
    final = lambda s: s.get("final_loss", s.get("loss_final"))
    for sigma in (0.0, 0.1):
        out = {}
        for fused in (True, False):
            cfg = _cfg(D0, sigma)
            cfg["execution"] = {"surface_fused": fused}
            cfg["stages"]["chamfer"]["num_iters"] = 25
            pose, betas, rt, tr = (t.clone().to(dev).requires_grad_(True) for t in (o_pose, o_betas, root, trans))
            optim_chamfer(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev),
                          root_orient=rt, trans=tr, img_mask=torch.ones(F, device=dev),
                          marker_labels=torch.zeros(F, M, dtype=torch.long, device=dev), smpl_inference=smpl, config=cfg)
            out[fused] = dict(last_stats("chamfer"))
        cf, cc = out[True], out[False]
        assert "loss_first" in cc and "first_loss" in cf      # (the composed route's statistics / the device solver's)
        print("OBS surface fused vs composed (sigma %g): %.6e -> %.6e / %.6e -> %.6e"
              % (sigma, first(cf), final(cf), first(cc), final(cc)))
        assert first(cf) == pytest.approx(first(cc), rel=1e-5)
        assert final(cf) == pytest.approx(final(cc), rel=5e-2)
        assert final(cf) < first(cf)


def test_composed_operator_gradient_matches_the_fused_closure(smpl, tables, dev):
    """losses.surface_chamfer_distance through SmplInference's backward gives the fused closure's data gradient (priors off) at
    one point: the two routes differ only in the vertex buffer the pick runs on and in summation order."""
    from uuo_mocap_amd.engine import ChamferProblem
    from uuo_mocap_amd.losses import surface_chamfer_distance
    from uuo_mocap_amd.optimization import get_marker_mask
    from uuo_mocap_amd.transforms import compute_root_orient_z, normalize_rot

    F, M = 5, 17
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 903, num_markers=M)
    cfg = _cfg(D0, 0.1)
    cfg["stages"]["chamfer"]["losses"].update(reg_pose_body=0.0, reg_betas=0.0)
    md = markers.to(dev)
    prob = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg)
    x = prob.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    loss, grad, _ = prob.evaluate(x)
    leaves = [t.clone().to(dev).requires_grad_(True) for t in (tp, zp, bp, pp)]
    t_, z_, b_, p_ = leaves
    out = smpl(poses=normalize_rot(p_), betas=torch.repeat_interleave(b_, dim=0, repeats=F),
               root_orient=normalize_rot(compute_root_orient_z(z_) @ root.to(dev)), trans=t_)
    lc = surface_chamfer_distance(md, out["vertices"], get_marker_mask(md), smpl, D0, 0.1)[0] * 10.0
    lc.backward()
    gc = torch.cat([t.grad.reshape(-1) for t in leaves]).cpu().numpy()
    print("OBS surface composed operator vs fused closure: loss rel %.2e, gradient rel %.2e"
          % (abs(float(lc) - loss) / loss, _rel_err(gc, grad.cpu().numpy())))
    assert float(lc) == pytest.approx(loss, rel=1e-5)
    assert _rel_err(gc, grad.cpu().numpy()) < 2e-4


# ------------------------------------------------------------------------------------------------ 4. off is off
def test_switched_off_is_bit_identical_with_and_without_faces(smpl, tables, dev):
    """The plain chamfer closure on a model that never got faces, on the same model after uuo_model_set_faces, and on a
    workspace that has just evaluated the surface term: loss and gradient bit for bit."""
    from uuo_mocap_amd.engine import ChamferProblem, DeviceModel

    F, M = 41, 50
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 123)
    args = (markers.to(dev), o_pose.to(dev), o_betas.to(dev), root.to(dev))
    plain = packaged_config("video_mocap")
    got = {}

    def on_fresh_thread():  # workspaces are per thread: these have never seen the term
        class _Bare:
            device_model = DeviceModel(dataclasses.replace(tables, faces=None), dev)

        assert not _Bare.device_model.has_faces
        p = ChamferProblem(_Bare, *args, plain)
        x = p.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
        got["bare"] = p.evaluate(x)
        with pytest.raises(RuntimeError, match="needs a body model with faces"):
            ChamferProblem(_Bare, *args, _cfg())
        rc = p.lib.uuo_fit_set_surface(p.fit, 1, ctypes.c_float(D0))
        assert rc != 0 and b"uuo_model_set_faces" in p.lib.uuo_last_error()
        f32 = np.ascontiguousarray(tables.faces, np.int32)
        assert p.lib.uuo_model_set_faces(_Bare.device_model.handle, f32.ctypes.data, int(f32.shape[0])) == 0
        got["faces"] = p.evaluate(x)
        torch.cuda.synchronize()

    t = threading.Thread(target=on_fresh_thread)
    t.start()
    t.join()
    assert "faces" in got
    (lb, gb, nb), (lf, gf, nf) = got["bare"], got["faces"]
    assert lb == lf and torch.equal(gb, gf) and torch.equal(nb, nf)
    ps, pp_ = ChamferProblem(smpl, *args, _cfg()), ChamferProblem(smpl, *args, plain)
    x = pp_.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    ls, gs, ns = ps.evaluate(x)                       # the term on this thread's workspace first
    l0, g0, n0 = pp_.evaluate(x)
    assert l0 == lb and torch.equal(g0, gb) and torch.equal(n0, nb)
    assert ls != l0 and not torch.equal(gs, g0) and torch.equal(ns, n0)
    # a key with weight 0 is the key absent
    zero = packaged_config("video_mocap")
    zero["stages"]["chamfer"]["losses"]["surface_chamfer"] = 0.0
    zero["stages"]["chamfer"]["surface_distance"] = D0
    lz, gz, _ = ChamferProblem(smpl, *args, zero).evaluate(x)
    assert lz == lb and torch.equal(gz, gb)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_library_and_routes_refuse_what_is_not_built(smpl, tables, dev):
    from uuo_mocap_amd import _lib
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem, PartProblem, current_stream, solve_batch

    F, M = 6, 12
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 55, num_markers=M)
    md = markers.to(dev)
    args = (md, o_pose.to(dev), o_betas.to(dev))
    lib = smpl.device_model.lib
    on = lambda fit, d0=D0: lib.uuo_fit_set_surface(fit, 1, ctypes.c_float(d0))
    err = lambda: lib.uuo_last_error().decode()

    def raw_eval(p, x):  # (evaluate() would re-arm the workspace from the problem's own settings)
        loss = torch.empty(1, device=dev)
        grad = torch.empty(p.n, device=dev)
        return lib.uuo_closure_eval(p.fit, current_stream(dev), ctypes.byref(p.problem), x.data_ptr(), loss.data_ptr(),
                                    grad.data_ptr(), None)

    pc = ChamferProblem(smpl, *args, root.to(dev), packaged_config("video_mocap"))
    xc = pc.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    try:
        for bad in (-1e-3, float("nan"), float("inf")):
            assert on(pc.fit, bad) != 0 and "surface_distance" in err(), bad
        assert lib.uuo_fit_set_surface(pc.fit, 2, ctypes.c_float(0.0)) != 0 and "0 (off) or 1" in err()
        # the marker and part stages (they share the (F, M) workspace of this thread)
        vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
        pm = MarkerProblem(smpl, *args, vids.to(dev), packaged_config("video_mocap"))
        xm = pm.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
        assert on(pm.fit) == 0
        assert raw_eval(pm, xm) != 0 and "chamfer stage only" in err()
        pt = PartProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), torch.arange(400, 900), packaged_config("video_mocap"))
        xt = pt.pack(torch.zeros(1, device=dev), tp.to(dev), bp.to(dev))
        assert on(pt.fit) == 0
        assert raw_eval(pt, xt) != 0 and "chamfer stage only" in err()
        # the soft-assignment data term
        soft = packaged_config("video_mocap")
        soft["stages"]["chamfer"]["losses"]["soft_chamfer"] = 1.0
        psf = ChamferProblem(smpl, *args, root.to(dev), soft)
        assert on(psf.fit) == 0
        assert raw_eval(psf, xc) != 0 and "soft-assignment" in err()
        # shared-betas solves
        assert on(pc.fit) == 0
        opt = _lib.UuoLbfgsOptions(3, 100, 0.1, 1e-7, 1e-9, 0, 0)
        stats = _lib.UuoLbfgsStats()

        def gather(user, mine, n, out):
            for i in range(n):
                out[i] = mine[i]
            return 0

        sh = _lib.UuoShared(_lib.GATHER_FN(gather), None, 0, 1)
        rc = lib.uuo_lbfgs_solve_shared(pc.fit, current_stream(dev), ctypes.byref(pc.problem), xc.clone().data_ptr(),
                                        ctypes.byref(opt), ctypes.byref(stats), ctypes.byref(sh), None, None)
        assert rc != 0 and "shared-betas solves do not carry the point-to-surface" in err()
    finally:
        assert lib.uuo_fit_set_surface(pc.fit, 0, ctypes.c_float(0.0)) == 0
    torch.cuda.synchronize()
    # the Python routes
    ps = ChamferProblem(smpl, *args, root.to(dev), _cfg())
    with pytest.raises(NotImplementedError, match="lock-step batches do not carry the point-to-surface"):
        solve_batch([ps], [xc.clone()], max_iter=2)

    class _Reducer:
        world = 1

    with pytest.raises(NotImplementedError, match="shared-betas solves do not carry the point-to-surface"):
        ps.solve_shared(xc.clone(), _Reducer(), max_iter=2)
    # no evaluation of the term on a workspace yet -> no corners to copy (a fresh thread's workspace)
    seen = {}

    def fresh():
        p = ChamferProblem(smpl, *args, root.to(dev), _cfg())
        try:
            p.surface_corners()
        except RuntimeError as exc:
            seen["msg"] = str(exc)

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert "no surface-term evaluation" in seen.get("msg", "")


# ------------------------------------------------------------------------------------------------ 6. the fit
def test_surface_config_fit_does_not_regress(smpl, oracle_smpl, tables, dev, record_property):
    """300 x 50 synthetic sequence (seed 0, as test_gpu_robust's fit): video_mocap_surface.yaml against video_mocap.yaml.  The
    surface fit's mean vertex error may exceed the plain fit's by at most 0.5 mm (the robust test's non-regression margin);
    every chamfer solve terminates normally with a finite evaluation count.  Measured figures: DESIGN.md section 4p."""
    from uuo_mocap_amd import multimodal
    from uuo_mocap_amd.engine import STOP_REASONS

    seq = make_sequence(tables, seed=0, num_frames=300, num_markers=50)
    pts = np.asarray(seq.markers.get_points()).copy()
    gt = torch.from_numpy(seq.gt["verts"])
    faces = torch.from_numpy(np.asarray(tables.faces).astype(np.int64)).to(dev)
    mk = torch.from_numpy(np.nan_to_num(pts)).float().to(dev)
    seen = torch.from_numpy(~np.isnan(pts).any(-1))
    res = {}
    for name in ("video_mocap", "video_mocap_surface"):
        out = multimodal.multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(pts.copy(), 30.0), dev,
                                                packaged_config(name), offset=0, print_options=[], save_stages=False,
                                                smpl_inference=smpl)
        v = oracle_smpl(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                        out["trans"].cpu().float())["vertices"]
        err = float((v - gt).norm(dim=-1).mean())
        dist = smpl.device_model.mesh_closest_points(v.to(dev).contiguous(), faces, mk)[0].cpu()
        m2s = float(dist[seen].mean())
        chamfer = list(multimodal.last_run_stats()["chamfer"])
        res[name] = (err, m2s, chamfer)
        record_property("v2v_%s_m" % name, err)
        record_property("marker_to_surface_%s_m" % name, m2s)
    (e0, s0, c0), (e1, s1, c1) = res["video_mocap"], res["video_mocap_surface"]
    print("OBS surface fit: mean vertex error plain %.2f mm surface %.2f mm; marker-to-surface distance plain %.2f mm surface "
          "%.2f mm; chamfer evaluations plain %s surface %s; stop reasons %s"
          % (1e3 * e0, 1e3 * e1, 1e3 * s0, 1e3 * s1, [c["n_eval"] for c in c0], [c["n_eval"] for c in c1],
             sorted({c["stop_reason"] for c in c1})))
    assert len(c1) >= 1
    for c in c1:
        assert math.isfinite(c["n_eval"]) and 0 < c["n_eval"] <= 12500, c          # max_eval = num_iters * 5 / 4
        assert math.isfinite(c["final_loss"]) and c["final_loss"] < c["first_loss"], c
        assert c["stop_reason"] in STOP_REASONS, c
    assert e1 <= e0 + 5e-4, (e0, e1)
