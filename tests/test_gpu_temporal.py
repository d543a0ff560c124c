"""EXTENSION: the joint-acceleration smoothness term (stages.{chamfer,marker}.losses.joint_accel, uuo_fit_set_joint_accel) on
the MI355X -- the fused closures against float64 autograd through the oracle's SMPL, the compact packing, the term switched
off, the operator-composed route, the routing rules and a fit through a stretch of frames without markers."""
import copy
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_support import (W_ACCEL_C as W_CHAMFER, W_ACCEL_M as W_MARKER, _fit_points as _fit, _inputs, _rel_err,  # noqa: E402,F401
                         _three_corners, dev, smpl, smpl64)
from stage_ref64 import ref_chamfer64 as _ref_chamfer, ref_marker64  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

M = 50
# W_CHAMFER, W_MARKER (10, 1), the weights of the parity checks: the term is then of the data term's size at the inputs below


def _ref_marker(smpl64, cfg, *args):   # (no latent offsets in this file: the reference needs no model tables)
    return ref_marker64(smpl64, None, cfg, *args)


def _cfg(w_chamfer=0.0, w_marker=0.0, sigma=0.0, name="video_mocap"):
    cfg = packaged_config(name)
    if w_chamfer is not None:
        cfg["stages"]["chamfer"]["losses"]["joint_accel"] = w_chamfer
    if w_marker is not None:
        cfg["stages"]["marker"]["losses"]["joint_accel"] = w_marker
    for k in ("chamfer", "part", "marker"):
        cfg["stages"][k]["robust_sigma"] = sigma
    return cfg


# ------------------------------------------------------------------------------------------------ 1. closure parity
@pytest.mark.parametrize("F", [3, 7, 300])
def test_joint_accel_closures_match_float64_autograd(smpl, smpl64, tables, dev, F):
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 60 + F)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F)
    for sigma in (0.0, 0.05):
        cfg, cfg0 = _cfg(W_CHAMFER, W_MARKER, sigma), _cfg(0.0, 0.0, sigma)
        # chamfer stage
        prob = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg)
        prob0 = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg0)
        assert prob.joint_accel == W_CHAMFER and prob0.joint_accel == 0.0
        x = prob.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
        loss, grad, nn = prob.evaluate(x)
        _, grad0, nn0 = prob0.evaluate(x)
        assert torch.equal(nn, nn0), "the term must not change the assignment"
        lo, g_ref = _ref_chamfer(smpl64, cfg, markers, o_pose, o_betas, root, x, nn)
        np.testing.assert_allclose(loss, lo, rtol=2e-5)
        assert _rel_err(grad.cpu().numpy(), g_ref) < 2e-4, ("chamfer", sigma)
        assert _rel_err(grad.cpu().numpy(), grad0.cpu().numpy()) > 1e-2, "the term must matter at these inputs"

        # marker stage: one-hot placement (plain and robust), three-corner placement (plain and robust: k_bary_fwd_r)
        xm = None
        for assign, bary in ((vids, None), (i3, b3)):
            pm = MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), assign.to(dev), cfg,
                               bary=None if bary is None else bary.to(dev))
            pm0 = MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), assign.to(dev), cfg0,
                                bary=None if bary is None else bary.to(dev))
            if xm is None:
                xm = pm.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
            lm, gm, _ = pm.evaluate(xm)
            _, gm0, _ = pm0.evaluate(xm)
            lo, g_ref = _ref_marker(smpl64, cfg, markers, o_pose, o_betas, xm, assign, bary)
            tag = ("three-corner" if bary is not None else "one-hot", sigma)
            np.testing.assert_allclose(lm, lo, rtol=2e-5, err_msg=str(tag))
            assert _rel_err(gm.cpu().numpy(), g_ref) < 2e-4, tag
            assert _rel_err(gm.cpu().numpy(), gm0.cpu().numpy()) > 1e-2, tag


def test_short_sequences_have_no_term(smpl, tables, dev):
    """F < 3: no second differences -- the closures equal the ones without the term, bit for bit."""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    for F in (1, 2):
        seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 90 + F)
        md = markers.to(dev)
        vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32).to(dev)
        pc, pc0 = (ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), c) for c in (_cfg(5.0, 5.0), _cfg()))
        x = pc.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
        (l1, g1, _), (l0, g0, _) = pc.evaluate(x), pc0.evaluate(x)
        assert l1 == l0 and torch.equal(g1, g0)
        pm, pm0 = (MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), vids, c) for c in (_cfg(5.0, 5.0), _cfg()))
        xm = pm.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
        (l1, g1, _), (l0, g0, _) = pm.evaluate(xm), pm0.evaluate(xm)
        assert l1 == l0 and torch.equal(g1, g0)


# ------------------------------------------------------------------------------------------------ 2. compact packing
def test_third_rows_get_no_gradient_from_the_term(smpl, tables, dev):
    """The term reaches the raw rotations through the Gram-Schmidt backward only: with reg_pose_body 0 the third rows' gradient
    entries are exact zeros (the solver's compact packing, DESIGN section 4c, stays exact) and a solve on the compact packing
    moves none of them."""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    F = 37
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 11)
    md = markers.to(dev)
    cfg = _cfg(W_CHAMFER, W_MARKER)
    cfg["stages"]["chamfer"]["losses"]["reg_pose_body"] = 0.0
    cfg["stages"]["marker"]["losses"]["reg_pose_body"] = 0.0
    pc = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg)
    x = pc.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    _, g, _ = pc.evaluate(x)
    gp = g[4 * F + 10:].reshape(F, 23, 3, 3)
    assert gp[:, :, :2].abs().sum() > 0 and not gp[:, :, 2].any()
    third = x[4 * F + 10:].reshape(F, 23, 3, 3)[:, :, 2].clone()
    pc.solve(x, max_iter=10, lr=0.1)
    assert torch.equal(x[4 * F + 10:].reshape(F, 23, 3, 3)[:, :, 2], third)

    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32).to(dev)
    pm = MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), vids, cfg)
    xm = pm.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
    _, g, _ = pm.evaluate(xm)
    gp = g[:207 * F].reshape(F, 23, 3, 3)
    groot = g[207 * F + 10:216 * F + 10].reshape(F, 3, 3)
    assert gp[:, :, :2].abs().sum() > 0 and not gp[:, :, 2].any() and not groot[:, 2].any()


# ------------------------------------------------------------------------------------------------ 3. off means off
def test_weight_zero_and_absent_are_bit_identical_and_workspaces_forget_the_term(smpl, tables, dev):
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    F = 41
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 23)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32).to(dev)
    i3, b3 = _three_corners(tables, seq, 5)
    absent = packaged_config("video_mocap")
    for k in ("chamfer", "marker"):
        assert "joint_accel" not in absent["stages"][k]["losses"]
    makers = {
        "chamfer": (lambda c: ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), c),
                    lambda p: p.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))),
        "marker": (lambda c: MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), vids, c),
                   lambda p: p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))),
        "marker3": (lambda c: MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), i3.to(dev), c, bary=b3.to(dev)),
                    lambda p: p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))),
    }
    for name, (make, pack) in makers.items():
        # a fresh workspace: a thread of its own (workspaces are per thread)
        fresh = {}

        def on_fresh_thread():
            p = make(absent)
            fresh["r"] = p.evaluate(pack(p), want_nn=False)[:2]
            torch.cuda.synchronize()

        t = threading.Thread(target=on_fresh_thread)
        t.start()
        t.join()
        pa, p0, pw = make(absent), make(_cfg(0.0, 0.0)), make(_cfg(W_CHAMFER, W_MARKER))
        x = pack(pa)
        lw, gw, _ = pw.evaluate(x, want_nn=False)           # the term on this thread's workspace first
        la, ga, _ = pa.evaluate(x, want_nn=False)           # then the same workspace without it
        l0, g0, _ = p0.evaluate(x, want_nn=False)
        assert la == l0 and torch.equal(ga, g0), name
        lf, gf = fresh["r"]
        assert la == lf and torch.equal(ga, gf), name
        assert lw > la, name


# ------------------------------------------------------------------------------------------------ 4. fused vs composed
def test_fused_and_composed_joint_accel_solves_agree(smpl, tables, dev):
    """25 L-BFGS iterations of the chamfer and the marker stage on the fused closures and on the operator-composed ones
    (execution.temporal_fused: False), with and without the robust data term: the start must agree to 1e-5 and the end to the
    tolerances of test_fused_and_composed_robust_solves_agree."""
    from uuo_mocap_amd.optimization import last_stats, optim_chamfer, optim_markers

    F = 37
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 21)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), vids.to(dev)] = 1.0
    first = lambda s: s.get("first_loss", s.get("loss_first"))
    final = lambda s: s.get("final_loss", s.get("loss_final"))
    for sigma in (0.0, 0.05):
        out = {}
        for fused in (True, False):
            cfg = _cfg(W_CHAMFER, W_MARKER, sigma)
            cfg["execution"] = {"temporal_fused": fused}
            for k in ("chamfer", "marker"):
                cfg["stages"][k]["num_iters"] = 25
            pose, betas, rt, tr = (t.clone().to(dev).requires_grad_(True) for t in (o_pose, o_betas, root, trans))
            optim_chamfer(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev),
                          root_orient=rt, trans=tr, img_mask=torch.ones(F, device=dev),
                          marker_labels=torch.zeros(F, M, dtype=torch.long, device=dev), smpl_inference=smpl, config=cfg)
            sc = dict(last_stats("chamfer"))
            o_pose_m = pose.detach().clone()
            optim_markers(md, pose_body=pose, o_pose_body=o_pose_m, betas=betas, o_betas=o_betas.to(dev), root_orient=rt,
                          trans=tr, barycentric_coords_one_hot=one_hot, img_mask=torch.ones(F, device=dev),
                          smpl_inference=smpl, config=cfg)
            out[fused] = (sc, dict(last_stats("marker")))
        (cf, mf), (cc, mc) = out[True], out[False]
        assert "loss_first" in cc and "loss_first" in mc and "first_loss" in cf   # (the composed route's statistics)
        print("OBS joint_accel fused vs composed (sigma %g): chamfer %.6e -> %.6e / %.6e -> %.6e; marker %.6e -> %.6e / "
              "%.6e -> %.6e" % (sigma, first(cf), final(cf), first(cc), final(cc), first(mf), final(mf), first(mc), final(mc)))
        assert first(cf) == pytest.approx(first(cc), rel=1e-5)
        assert final(cf) == pytest.approx(final(cc), rel=5e-2)
        assert final(mf) == pytest.approx(final(mc), rel=8e-2)
        assert final(cf) < first(cf) and final(mf) < first(mf)


# ------------------------------------------------------------------------------------------------ 5. routing
def test_lockstep_hypotheses_with_the_term_match_the_threaded_route(smpl, tables, dev):
    """hypothesis_lockstep: True cannot batch the term (lockstep_supported is False): the hypotheses run on threads and the
    fit is the threaded route's, bit for bit."""
    from uuo_mocap_amd.multimodal import multimodal_video_mocap

    seq = make_sequence(tables, seed=4, num_frames=24, num_markers=16)
    cfg = _cfg(W_CHAMFER, W_MARKER)
    for k in ("chamfer", "marker", "part"):
        cfg["stages"][k]["num_iters"] = 30
    outs = []
    for lock in (True, False):
        outs.append(multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(seq.markers.get_points().copy(), 30.0),
                                           dev, copy.deepcopy(cfg), offset=0, print_options=[], save_stages=False,
                                           smpl_inference=smpl, execution={"hypothesis_lockstep": lock}))
    for key in ("pose_body", "betas", "root_orient", "trans"):
        assert torch.equal(torch.as_tensor(outs[0][key]), torch.as_tensor(outs[1][key])), key


def test_marker_frame_sharding_and_lockstep_batches_refuse_the_term(smpl, tables, dev):
    from uuo_mocap_amd import parallel
    from uuo_mocap_amd.engine import ChamferProblem, solve_batch
    from uuo_mocap_amd.optimization import optim_markers

    F = 9
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 3)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), vids.to(dev)] = 1.0
    pose, betas, rt, tr = (t.clone().to(dev) for t in (o_pose, o_betas, root, trans))
    with parallel.shard_frames(joint_with_one_rank=True):
        with pytest.raises(NotImplementedError, match="frame-block sharding"):
            optim_markers(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev), root_orient=rt,
                          trans=tr, barycentric_coords_one_hot=one_hot, img_mask=torch.ones(F, device=dev),
                          smpl_inference=smpl, config=_cfg(W_CHAMFER, W_MARKER))
    p = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), _cfg(W_CHAMFER, W_MARKER))
    x = p.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    with pytest.raises(NotImplementedError, match="lock-step"):
        solve_batch([p], [x], max_iter=3)


def test_library_refuses_the_term_for_the_part_stage(smpl, tables, dev):
    from uuo_mocap_amd.engine import PartProblem

    F = 9
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 8)
    vlabels = torch.argmax(smpl.get_lbs_weights(), dim=-1)
    vidx = torch.cat([(vlabels == j).nonzero(as_tuple=True)[0] for j in (0, 1, 4, 7, 10)]).to(dev)
    pp = PartProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), root.to(dev), vidx, packaged_config("video_mocap"))
    x = pp.pack(torch.zeros(1, 1, 1, device=dev), trans.to(dev), o_betas.to(dev))
    loss0 = pp.evaluate(x)[0]
    pp.joint_accel = 1.0  # what no config can produce: the library itself must refuse it
    with pytest.raises(RuntimeError, match="part stage"):
        pp.evaluate(x)
    pp.joint_accel = 0.0
    assert pp.evaluate(x)[0] == loss0
    lib = smpl.device_model.lib
    assert lib.uuo_fit_set_joint_accel(pp.fit, -1.0) != 0 and lib.uuo_fit_set_joint_accel(pp.fit, float("nan")) != 0


# ------------------------------------------------------------------------------------------------ 6. gap fill
GAP0, GAP_LEN = 144, 12


def _errors(out, seq, oracle_smpl):
    from uuo_mocap_amd.metrics import compute_accel_error

    r = oracle_smpl(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                    out["trans"].cpu().float())
    gt = torch.from_numpy(seq.gt["verts"])
    per_frame = (r["vertices"] - gt).norm(dim=-1).mean(dim=1)
    gt_j = torch.from_numpy(np.asarray(seq.gt["joints"]))[:, :24].float()
    return per_frame, float(compute_accel_error(r["joints"][:, :24], gt_j, 30.0))


def test_gap_fill_smooth_config(smpl, oracle_smpl, tables, dev, record_property):
    """300 x 50 synthetic sequence with every marker missing in 12 consecutive mid-sequence frames.  video_mocap_smooth.yaml must
    carry the body through the gap at most half as far from the ground truth as video_mocap.yaml, cost at most 0.5 mm of mean
    vertex error on the clean sequence, and lower its acceleration error.  The thresholds were set from the first measured run
    with margin: gap frames 664.6 mm plain, 8.8 mm smooth; clean 6.73 / 5.04 mm; clean acceleration
    error 13.0 / 0.62 m/s^2."""
    seq = make_sequence(tables, seed=0, num_frames=300, num_markers=M)
    clean = np.asarray(seq.markers.get_points()).copy()
    gap = clean.copy()
    gap[GAP0:GAP0 + GAP_LEN] = 0.0
    res = {}
    for tag, pts in (("gap", gap), ("clean", clean)):
        for name in ("video_mocap", "video_mocap_smooth"):
            res[(tag, name)] = _errors(_fit(seq, pts, name, smpl, dev), seq, oracle_smpl)
    g_plain = float(res[("gap", "video_mocap")][0][GAP0:GAP0 + GAP_LEN].mean())
    g_smooth = float(res[("gap", "video_mocap_smooth")][0][GAP0:GAP0 + GAP_LEN].mean())
    c_plain, c_smooth = (float(res[("clean", n)][0].mean()) for n in ("video_mocap", "video_mocap_smooth"))
    a_plain, a_smooth = (res[("clean", n)][1] for n in ("video_mocap", "video_mocap_smooth"))
    for k, v in (("gap_plain_m", g_plain), ("gap_smooth_m", g_smooth), ("clean_plain_m", c_plain),
                 ("clean_smooth_m", c_smooth), ("accel_plain", a_plain), ("accel_smooth", a_smooth)):
        record_property(k, v)
    print("OBS gap fill: gap-frame vertex error plain %.2f mm smooth %.2f mm; clean all-frame plain %.2f mm smooth %.2f mm; "
          "clean accel error plain %.3f smooth %.3f m/s^2" % (1e3 * g_plain, 1e3 * g_smooth, 1e3 * c_plain, 1e3 * c_smooth,
                                                             a_plain, a_smooth))
    assert g_smooth <= 0.5 * g_plain, res
    assert g_smooth < 2e-2, res
    assert c_smooth <= c_plain + 5e-4, res
    assert a_smooth < 0.25 * a_plain, res
