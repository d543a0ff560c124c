"""EXTENSION: latent per-marker offsets in the fused marker stage (stages.marker.losses.latent_offsets, uuo_problem_t.w_offsets)
on the MI355X -- the closures against float64 autograd, the start value, the term switched off, the compact packing,
determinism, recovery of the generator's offsets and the fit quality of video_mocap_offsets.yaml."""
import copy
import ctypes
import os
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

from gpu_support import W_ACCEL_M as W_ACCEL, W_OFFS, _rel_err, _three_corners, _vertex_error, dev, smpl  # noqa: E402,F401
from oracle import stages_ref  # noqa: E402
from stage_ref64 import _float64, _skin64  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.engine import MARKER_DISTANCE  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

M = 50
# W_OFFS, W_ACCEL (2, 1), the weights of the parity checks: both terms then matter at the inputs below
STANDOFF = dict(standoff_tilt_deg=30.0, standoff_mm=(8.0, 14.0))


def _cfg(w_offs=W_OFFS, sigma=0.0, accel=0.0):
    cfg = packaged_config("video_mocap")
    st = cfg["stages"]["marker"]
    if w_offs is not None:
        st["losses"]["latent_offsets"] = w_offs
    if accel:
        st["losses"]["joint_accel"] = accel
    st["robust_sigma"] = sigma
    return cfg


def _inputs(tables, F, seed):
    seq = make_sequence(tables, seed=seed, num_frames=F, num_markers=M)
    markers = torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float()
    o_pose = seq.img_smpl.pose_body.clone().float()
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).float()
    root = seq.img_smpl.root_orient.clone().float()
    trans = torch.median(markers, dim=1)[0].clone()
    gen = torch.Generator().manual_seed(seed + 2)
    r = lambda *s: torch.randn(*s, generator=gen)
    d = r(M, 3)
    offs = (MARKER_DISTANCE * (1.0 + 0.3 * r(M, 1))) * d / d.norm(dim=1, keepdim=True)
    pert = (o_pose + 0.05 * r(F, 23, 3, 3), o_betas + 0.3 * r(1, 10), root + 0.05 * r(F, 1, 3, 3), trans + 0.02 * r(F, 3),
            offs)
    return seq, markers, o_pose, o_betas, root, trans, pert


def _ref(tables, cfg, markers, o_pose, o_betas, x, assign, bary=None):
    """Loss and gradient of the marker stage with latent offsets in float64 torch autograd, parameters
    [pose 207F | betas 10 | root 9F | trans 3F | offsets 3M]."""
    F = markers.shape[0]
    st = cfg["stages"]["marker"]
    w, sigma = st["losses"], float(st.get("robust_sigma", 0.0))
    with _float64():
        x = x.detach().cpu().double()
        markers, o_pose, o_betas = (t.detach().cpu().double() for t in (markers, o_pose, o_betas))
        n0 = 219 * F + 10
        leaves = [t.clone().requires_grad_(True) for t in (
            x[:207 * F].reshape(F, 23, 3, 3), x[207 * F:207 * F + 10].reshape(1, 10),
            x[207 * F + 10:216 * F + 10].reshape(F, 1, 3, 3), x[216 * F + 10:n0].reshape(F, 3), x[n0:].reshape(M, 3))]
        pose, betas, root, trans, offs = leaves
        rot = torch.cat([stages_ref.normalize_rot(root), stages_ref.normalize_rot(pose)], dim=1)
        a = assign.cpu().long().reshape(M, -1)
        K = a.shape[1]
        vp, T_R, T_t, joints = _skin64(tables, rot, betas, trans, a.reshape(-1))
        pts = vp.reshape(F, M, K, 3) + offs[None, :, None]
        vk = torch.einsum("fmkab,fmkb->fmka", T_R.reshape(F, M, K, 3, 3), pts) + T_t.reshape(F, M, K, 3)
        b = torch.ones(M, 1, dtype=torch.float64) if bary is None else bary.cpu().double()
        vm = (vk * b[None, :, :, None]).sum(2)
        s = ((markers - vm) ** 2).sum(-1)
        rho = s * (sigma * sigma / (sigma * sigma + s)) if sigma else s
        mask = stages_ref.get_marker_mask(markers).double()
        loss = torch.mean(rho * mask) * w["marker"] + Fn.mse_loss(pose, o_pose) * w["reg_pose_body"] + \
            Fn.mse_loss(betas, o_betas) * w["reg_betas"] + \
            torch.mean((offs.norm(dim=1) - MARKER_DISTANCE) ** 2) * w["latent_offsets"]
        if w.get("joint_accel", 0.0) and F >= 3:
            acc = joints[:-2] - 2.0 * joints[1:-1] + joints[2:]
            loss = loss + Fn.mse_loss(acc, torch.zeros_like(acc)) * w["joint_accel"]
        loss.backward()
    return float(loss.detach()), torch.cat([t.grad.reshape(-1) for t in leaves]).numpy()


def _problem(smpl, dev, cfg, markers, o_pose, o_betas, assign, bary=None):
    from uuo_mocap_amd.engine import MarkerProblem

    return MarkerProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), assign.to(dev), cfg,
                         bary=None if bary is None else bary.to(dev))


# ------------------------------------------------------------------------------------------------ 1. float64 parity
@pytest.mark.parametrize("F", [1, 2, 7, 300])
def test_offset_closures_match_float64_autograd(smpl, tables, dev, F):
    seq, markers, o_pose, o_betas, root, trans, (pp, bp, rp, tp, op) = _inputs(tables, F, 70 + F)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F)
    for assign, bary in ((vids, None), (i3, b3)):
        for sigma in (0.0, 0.05):
            for accel in (0.0, W_ACCEL):
                cfg = _cfg(W_OFFS, sigma, accel)
                prob = _problem(smpl, dev, cfg, markers, o_pose, o_betas, assign, bary)
                assert prob.n == 219 * F + 10 + 3 * M
                x = prob.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev), op.to(dev))
                loss, grad, _ = prob.evaluate(x, want_nn=False)
                lo, g_ref = _ref(tables, cfg, markers, o_pose, o_betas, x, assign, bary)
                g = grad.cpu().numpy()
                tag = ("three-corner" if bary is not None else "one-hot", F, sigma, accel)
                eo = _rel_err(g[-3 * M:], g_ref[-3 * M:])
                print("OBS offsets parity %s: loss rel %.2e, gradient rel %.2e, offsets block rel %.2e"
                      % (tag, abs(loss - lo) / abs(lo), _rel_err(g, g_ref), eo))
                np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=str(tag))
                assert _rel_err(g, g_ref) < 2e-4, tag
                assert eo < 2e-4, tag


# ------------------------------------------------------------------------------------------------ 2. start value
def test_start_value_is_the_masked_mean_residual_in_the_marker_frame(smpl, tables, dev):
    """At o = 0, with the priors and the robust term off, the offsets' block of the gradient is
    -(2 w_data / (F M)) sum_f mask T_R^T (x - v) (three-corner: sum_k b_k T_R,k^T (x - vm)), in float64; offsets_start is
    MARKER_DISTANCE times its negative's unit vector, and 0 for a marker without a valid frame."""
    F = 23
    seq, markers, o_pose, o_betas, root, trans, (pp, bp, rp, tp, _) = _inputs(tables, F, 5)
    markers[:, 7] = 0.0   # marker 7 never seen
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, 3)
    cfg = _cfg(W_OFFS, 0.05, W_ACCEL)   # (offsets_start switches the robust and joint-acceleration terms off itself)
    for assign, bary in ((vids, None), (i3, b3)):
        prob = _problem(smpl, dev, cfg, markers, o_pose, o_betas, assign, bary)
        x = prob.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
        cfg0 = _cfg(W_OFFS)
        for k in ("reg_pose_body", "reg_betas"):
            cfg0["stages"]["marker"]["losses"][k] = 0.0
        p0 = _problem(smpl, dev, cfg0, markers, o_pose, o_betas, assign, bary)
        g_dev = p0.evaluate(x, want_nn=False)[1][-3 * M:].reshape(M, 3).cpu().double()
        with _float64():
            xd = x.detach().cpu().double()
            rot = torch.cat([stages_ref.normalize_rot(xd[207 * F + 10:216 * F + 10].reshape(F, 1, 3, 3)),
                             stages_ref.normalize_rot(xd[:207 * F].reshape(F, 23, 3, 3))], dim=1)
            a = assign.long().reshape(M, -1)
            K = a.shape[1]
            vp, T_R, T_t, _ = _skin64(tables, rot, xd[207 * F:207 * F + 10].reshape(1, 10), xd[216 * F + 10:219 * F + 10].reshape(F, 3),
                                      a.reshape(-1))
            vk = (torch.einsum("fkab,fkb->fka", T_R, vp) + T_t).reshape(F, M, K, 3)
            b = torch.ones(M, 1, dtype=torch.float64) if bary is None else b3.double()
            res = markers.double() - (vk * b[None, :, :, None]).sum(2)
            mask = stages_ref.get_marker_mask(markers.double()).double()
            TRt = T_R.reshape(F, M, K, 3, 3).transpose(-1, -2)
            g64 = -(2.0 / (F * M)) * torch.einsum("fm,fmk,fmkab,fmb->ma", mask, b.expand(M, K)[None].expand(F, M, K), TRt, res)
        err = _rel_err(g_dev.numpy(), g64.numpy())
        print("OBS start value gradient (%s): rel err %.2e" % ("one-hot" if bary is None else "three-corner", err))
        assert err < 2e-4
        assert not g_dev[7].any()
        o0 = prob.offsets_start(x).cpu().double()
        u = -g64 / g64.norm(dim=1, keepdim=True)
        keep = torch.arange(M) != 7
        np.testing.assert_allclose(o0[keep].numpy(), (MARKER_DISTANCE * u[keep]).numpy(), atol=1e-6)
        assert not o0[7].any()


# ------------------------------------------------------------------------------------------------ 3. off means off
def test_weight_zero_and_absent_are_bit_identical_and_workspaces_forget_the_term(smpl, tables, dev):
    from uuo_mocap_amd.engine import MarkerProblem

    F = 41
    seq, markers, o_pose, o_betas, root, trans, (pp, bp, rp, tp, op) = _inputs(tables, F, 23)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, 5)
    absent = packaged_config("video_mocap")
    assert "latent_offsets" not in absent["stages"]["marker"]["losses"]
    for assign, bary in ((vids, None), (i3, b3)):
        make = lambda c: _problem(smpl, dev, c, markers, o_pose, o_betas, assign, bary)
        fresh = {}

        def on_fresh_thread():   # a workspace of its own (workspaces are per thread)
            p = make(absent)
            xf = p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
            fresh["eval"] = p.evaluate(xf, want_nn=False)[:2]
            p.solve(xf, max_iter=20)
            fresh["solve"] = xf
            torch.cuda.synchronize()

        t = threading.Thread(target=on_fresh_thread)
        t.start()
        t.join()
        pa, p0, pw = make(absent), make(_cfg(0.0)), make(_cfg(W_OFFS))
        assert pa.n == p0.n == 219 * F + 10 and pw.n == pa.n + 3 * M
        assert not pa.has_offsets and not p0.has_offsets and len(p0.unpack(torch.zeros(p0.n))) == 4
        x = pa.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
        xw = pw.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev), op.to(dev))
        lw, gw, _ = pw.evaluate(xw, want_nn=False)          # the term on this thread's workspace first
        pw.solve(xw.clone(), max_iter=5)
        la, ga, _ = pa.evaluate(x, want_nn=False)           # then the same workspace without it
        l0, g0, _ = p0.evaluate(x, want_nn=False)
        tag = "three-corner" if bary is not None else "one-hot"
        assert la == l0 and torch.equal(ga, g0), tag
        lf, gf = fresh["eval"]
        assert la == lf and torch.equal(ga, gf), tag
        xa, x0 = x.clone(), x.clone()
        pa.solve(xa, max_iter=20)
        p0.solve(x0, max_iter=20)
        assert torch.equal(xa, x0) and torch.equal(xa, fresh["solve"]), tag
        assert lw != la, tag


# ------------------------------------------------------------------------------------------------ 4. packing, determinism
def test_compact_and_full_packings_agree_and_solves_are_deterministic(smpl, tables, dev):
    """The offsets extend the trans run of the compact packing (csrc/closure.hip uuo_stage_index_map).  Against the full packing
    (UUO_NO_COMPACT=1 in the debug flavour) a solve takes the same path; the third rows of the raw rotations keep exact-zero
    gradients; two identical solves are bit for bit equal."""
    from uuo_mocap_amd import _lib
    from uuo_mocap_amd._lib import UuoLbfgsOptions, UuoLbfgsStats
    from uuo_mocap_amd.engine import _ptr, current_stream

    dbg = _lib.load_debug()
    F = 37
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 31)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, 9)
    for assign, bary in ((vids, None), (i3, b3)):
        tag = "three-corner" if bary is not None else "one-hot"
        cfg = _cfg(W_OFFS, 0.05, W_ACCEL)
        cfg["stages"]["marker"]["losses"]["reg_pose_body"] = 0.0
        prob = _problem(smpl, dev, cfg, markers, o_pose, o_betas, assign, bary)
        x0 = prob.pack(o_pose.to(dev), o_betas.to(dev), root.to(dev), trans.to(dev))
        x0[219 * F + 10:] = prob.offsets_start(x0).reshape(-1)
        _, g, _ = prob.evaluate(x0, want_nn=False)
        gp = g[:207 * F].reshape(F, 23, 3, 3)
        groot = g[207 * F + 10:216 * F + 10].reshape(F, 3, 3)
        assert gp[:, :, :2].abs().sum() > 0 and not gp[:, :, 2].any() and not groot[:, 2].any(), tag
        assert g[-3 * M:].abs().sum() > 0, tag
        prob.problem.w_pose = 0.1   # (the prior back: the third rows sit on their targets, so the solve runs compact)

        def solve(no_compact):
            x = x0.clone()
            losses = []
            cb = _lib.EVAL_CALLBACK(lambda user, i, loss, d_x_eval: losses.append(loss))
            opt = UuoLbfgsOptions(60, 100, 1.0, 1e-7, 1e-9, 0, 0)
            st = UuoLbfgsStats()
            os.environ["UUO_NO_COMPACT"] = "1" if no_compact else "0"
            try:
                prob._arm()
                rc = dbg.uuo_lbfgs_solve(prob.fit, current_stream(dev), ctypes.byref(prob.problem), _ptr(x),
                                         ctypes.byref(opt), ctypes.byref(st), ctypes.cast(cb, ctypes.c_void_p), None)
            finally:
                os.environ.pop("UUO_NO_COMPACT", None)
            assert rc == 0, dbg.uuo_last_error()
            torch.cuda.synchronize()
            return x, losses, (st.n_iter, st.n_eval, st.stop_reason)

        xc, lc, sc = solve(False)
        xf, lf, sf = solve(True)
        head = min(len(lc), len(lf), 40)
        np.testing.assert_allclose(lc[:head], lf[:head], rtol=1e-6, err_msg=tag)
        assert abs(sc[0] - sf[0]) <= 2 and abs(sc[1] - sf[1]) <= 3, (tag, sc, sf)
        assert float((xc - xf).abs().max()) < 1e-3, tag
        assert not torch.equal(xc[-3 * M:], x0[-3 * M:]), tag
        xc2, lc2, sc2 = solve(False)
        assert torch.equal(xc, xc2) and lc == lc2 and sc == sc2, tag
        xa, xb = x0.clone(), x0.clone()
        prob.solve(xa, max_iter=30)
        prob.solve(xb, max_iter=30)
        assert torch.equal(xa, xb), tag


# ------------------------------------------------------------------------------------------------ 5. routes
def test_library_and_routes_refuse_the_term_where_it_is_not_built(smpl, tables, dev):
    from uuo_mocap_amd.engine import ChamferProblem, solve_batch
    from uuo_mocap_amd.optimization import lockstep_supported, optim_markers

    F = 9
    seq, markers, o_pose, o_betas, root, trans, (pp, bp, rp, tp, op) = _inputs(tables, F, 8)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    prob = _problem(smpl, dev, _cfg(W_OFFS), markers, o_pose, o_betas, vids)
    x = prob.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev), op.to(dev))
    with pytest.raises(NotImplementedError, match="latent"):
        solve_batch([prob], [x], max_iter=3)
    assert not lockstep_supported(_cfg(W_OFFS), "marker") and lockstep_supported(_cfg(0.0), "marker")
    pc = ChamferProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), root.to(dev), packaged_config("video_mocap"))
    xc = pc.pack(tp.to(dev), torch.zeros(F, 1, 1, device=dev), bp.to(dev), pp.to(dev))
    pc.problem.w_offsets = 1.0   # what no config can produce: the library itself must refuse it
    with pytest.raises(RuntimeError, match="marker stage only"):
        pc.evaluate(xc)
    pc.problem.w_offsets = 0.0
    pc.evaluate(xc)
    prob.problem.w_offsets = -1.0
    with pytest.raises(RuntimeError, match="w_offsets"):
        prob.evaluate(x)
    # the composed route (a row with four non-zeros) names the term
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), vids.long().to(dev)] = 1.0
    one_hot[0, :4] = 0.25
    leaves = [t.clone().to(dev).requires_grad_(True) for t in (o_pose, o_betas, root, trans)]
    with pytest.raises(NotImplementedError, match="latent_offsets"):
        optim_markers(markers.to(dev), pose_body=leaves[0], o_pose_body=o_pose.to(dev), betas=leaves[1],
                      o_betas=o_betas.to(dev), root_orient=leaves[2], trans=leaves[3], barycentric_coords_one_hot=one_hot,
                      img_mask=torch.ones(F, device=dev), smpl_inference=smpl, config=_cfg(W_OFFS))


# ------------------------------------------------------------------------------------------------ 6. recovery, quality
def _fit(seq, points, cfg, smpl, dev):
    from uuo_mocap_amd.multimodal import multimodal_video_mocap

    return multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(points.copy(), 30.0), dev, cfg, offset=0,
                                  print_options=[], save_stages=False, smpl_inference=smpl)


def test_offsets_recovery(smpl, tables, dev, record_property):
    """make_sequence(seed=0) places marker m at its vertex + T_R (9.5 mm along the outward direction) -- the model of the term
    with o_m = 0.0095 out_dir.  A marker-stage fit of video_mocap_offsets.yaml on the generator's own placement (from the
    HMR stand-in's noisy body pose with the true root) must find those offsets.  Bound from the first measured run with margin
    (DESIGN.md section 4n)."""
    from uuo_mocap_amd.optimization import optim_markers

    F = 300
    seq = make_sequence(tables, seed=0, num_frames=F, num_markers=M)
    markers = torch.from_numpy(np.nan_to_num(seq.markers.get_points())).float().to(dev)
    o_pose = seq.img_smpl.pose_body.clone().float().to(dev)
    o_betas = (seq.img_smpl.betas.sum(0, keepdim=True) / seq.img_smpl.img_mask.sum()).float().to(dev)
    root = torch.from_numpy(np.ascontiguousarray(seq.gt["rot"][:, :1])).float().to(dev)
    trans = torch.median(markers, dim=1)[0].clone()
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long().to(dev)
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), vids] = 1.0
    leaves = [t.clone().requires_grad_(True) for t in (o_pose, o_betas, root, trans)]
    offs = torch.full((M, 3), float("nan"), device=dev)
    optim_markers(markers, pose_body=leaves[0], o_pose_body=o_pose, betas=leaves[1], o_betas=o_betas, root_orient=leaves[2],
                  trans=leaves[3], barycentric_coords_one_hot=one_hot, img_mask=torch.ones(F, device=dev),
                  smpl_inference=smpl, config=packaged_config("video_mocap_offsets"), marker_offsets=offs)
    d = np.linalg.norm(offs.cpu().numpy() - np.asarray(seq.gt["marker_offsets"]), axis=1)
    record_property("recovery_mean_m", float(d.mean()))
    print("OBS offsets recovery on the generator's placement: mean %.3f mm, median %.3f mm, max %.3f mm"
          % (1e3 * d.mean(), 1e3 * np.median(d), 1e3 * d.max()))
    assert np.isfinite(d).all()
    assert d.mean() < 2e-3   # first measured run: 1.49 mm (median 1.40, max 4.46)


def test_offsets_config_quality_and_recovery(smpl, oracle_smpl, tables, dev, record_property):
    """video_mocap.yaml against video_mocap_offsets.yaml on the 300 x 50 seed-0 capture, clean (markers 9.5 mm along the
    outward direction) and stand-off (directions tilted up to 30 degrees, lengths 8-14 mm), by mean vertex error against the
    ground truth; and the fitted offsets against the generator's.  Thresholds from the first measured run with margin
    (DESIGN.md section 4n)."""
    res = {}
    for tag, kw in (("clean", {}), ("standoff", STANDOFF)):
        seq = make_sequence(tables, seed=0, num_frames=300, num_markers=M, **kw)
        pts = np.asarray(seq.markers.get_points()).copy()
        for name in ("video_mocap", "video_mocap_offsets"):
            out = _fit(seq, pts, packaged_config(name), smpl, dev)
            res[(tag, name)] = _vertex_error(out, seq, oracle_smpl)
            assert ("marker_offsets" in out) == (name == "video_mocap_offsets")
            if name == "video_mocap_offsets":
                offs = out["marker_offsets"].numpy()
                assert offs.shape == (M, 3) and np.isfinite(offs).all()
                true = np.asarray(seq.gt["marker_offsets"])
                d = np.linalg.norm(offs - true, axis=1)
                res[(tag, "recovery")] = (float(np.median(d)), float(d.mean()))
    for k, v in res.items():
        record_property("_".join(k), v)
    print("OBS offsets quality: clean plain %.2f mm offsets %.2f mm; stand-off plain %.2f mm offsets %.2f mm; offsets recovery "
          "(median, mean over all columns) clean %.2f / %.2f mm, stand-off %.2f / %.2f mm"
          % (1e3 * res[("clean", "video_mocap")], 1e3 * res[("clean", "video_mocap_offsets")],
             1e3 * res[("standoff", "video_mocap")], 1e3 * res[("standoff", "video_mocap_offsets")],
             1e3 * res[("clean", "recovery")][0], 1e3 * res[("clean", "recovery")][1],
             1e3 * res[("standoff", "recovery")][0], 1e3 * res[("standoff", "recovery")][1]))
    # first measured run (latent_offsets 0.1): clean 6.73 -> 4.15 mm, stand-off 6.57 -> 4.25 mm (0.65 x)
    assert res[("clean", "video_mocap_offsets")] <= res[("clean", "video_mocap")], res
    assert res[("clean", "video_mocap_offsets")] < 5.0e-3, res
    assert res[("standoff", "video_mocap_offsets")] <= 0.70 * res[("standoff", "video_mocap")], res
