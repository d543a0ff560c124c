"""EXTENSION: the contact-gated foot-lock term (stages.{chamfer,marker}.losses.foot_lock, uuo_fit_set_foot_lock) on the MI355X
-- the fused closures against float64 autograd, the term switched off, the compact packing, the operator-composed route, the
routing rules, and what video_mocap_contact.yaml buys on a capture with planted feet."""
import copy
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from foot_lock_ref64 import _cfg, _contacts  # noqa: E402
from gpu_support import (W_LOCK_C as W_CHAMFER, W_LOCK_M as W_MARKER, _fit_points as _fit, _inputs,  # noqa: E402,F401
                         _makers_contacts as _makers, _marker_x, _rel_err, _three_corners, dev, smpl, smpl64)
from stage_ref64 import ref_chamfer64 as _ref_chamfer, ref_marker64 as _ref_marker  # noqa: E402
from uuo_mocap_amd.config import packaged_config  # noqa: E402
from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence  # noqa: E402

M = 50
# W_CHAMFER, W_MARKER (100, 10), the weights of the parity checks.  At the inputs below (translation perturbed by 2 cm a frame, so
# feet that move ~3 cm a frame and data residuals of ~2 cm) the term's gradient on the translation, 2 w g v / (6 (F - 1)), is then
# of the size of the data term's, 2 w_data d / F: the check that the term matters (> 1e-2 of the gradient) is met with a wide margin.


# ------------------------------------------------------------------------------------------------ 6. closure parity
@pytest.mark.parametrize("F", [2, 3, 7, 300])
def test_foot_lock_closures_match_float64_autograd(smpl, smpl64, tables, dev, F):
    """Loss rtol 2e-5, gradient relative error < 2e-4 against float64 autograd, and the term changes the gradient by more than
    1e-2 relative -- chamfer, one-hot and three-corner marker closures; plain and robust; joint_accel off and on; latent
    offsets off and on for the marker closures."""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 160 + F)
    contacts = _contacts(F, F)
    assert float((contacts[1:] * contacts[:-1]).sum()) > 0
    if F >= 7:
        assert bool((contacts == 0).any())
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F)
    args = (md, o_pose.to(dev), o_betas.to(dev))
    for sigma in (0.0, 0.05):
        for accel in (False, True):
            cfg, cfg0 = _cfg(W_CHAMFER, W_MARKER, sigma, accel), _cfg(0.0, 0.0, sigma, accel)
            prob = ChamferProblem(smpl, *args, root.to(dev), cfg, foot_contacts=contacts)
            prob0 = ChamferProblem(smpl, *args, root.to(dev), cfg0, foot_contacts=contacts)
            assert prob.foot_lock == W_CHAMFER and prob0.foot_lock == 0.0
            x = prob.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
            loss, grad, nn = prob.evaluate(x)
            _, grad0, nn0 = prob0.evaluate(x)
            assert torch.equal(nn, nn0), "the term must not change the assignment"
            lo, g_ref = _ref_chamfer(smpl64, cfg, markers, o_pose, o_betas, root, x, nn, contacts)
            g = grad.cpu().numpy()
            tag = ("chamfer", F, sigma, accel)
            print("OBS foot_lock parity %s: loss rel %.2e, gradient rel %.2e, term's share of the gradient %.2e"
                  % (tag, abs(loss - lo) / abs(lo), _rel_err(g, g_ref), _rel_err(g, grad0.cpu().numpy())))
            np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=str(tag))
            assert _rel_err(g, g_ref) < 2e-4, tag
            assert _rel_err(g, grad0.cpu().numpy()) > 1e-2, tag

            for offs in (False, True):
                cfg, cfg0 = _cfg(W_CHAMFER, W_MARKER, sigma, accel, offs), _cfg(0.0, 0.0, sigma, accel, offs)
                for assign, bary in ((vids, None), (i3, b3)):
                    kw = {"bary": None if bary is None else bary.to(dev), "foot_contacts": contacts}
                    pm = MarkerProblem(smpl, *args, assign.to(dev), cfg, **kw)
                    pm0 = MarkerProblem(smpl, *args, assign.to(dev), cfg0, **kw)
                    assert pm.foot_lock == W_MARKER and pm0.foot_lock == 0.0 and pm.has_offsets == offs
                    xm = _marker_x(pm, pp, bp, rp, tp, dev, F)
                    lm, gm, _ = pm.evaluate(xm, want_nn=False)
                    _, gm0, _ = pm0.evaluate(xm, want_nn=False)
                    lo, g_ref = _ref_marker(smpl64, tables, cfg, markers, o_pose, o_betas, xm, assign, bary, contacts)
                    g = gm.cpu().numpy()
                    tag = ("three-corner" if bary is not None else "one-hot", F, sigma, accel, offs)
                    print("OBS foot_lock parity %s: loss rel %.2e, gradient rel %.2e, term's share of the gradient %.2e"
                          % (tag, abs(lm - lo) / abs(lo), _rel_err(g, g_ref), _rel_err(g, gm0.cpu().numpy())))
                    np.testing.assert_allclose(lm, lo, rtol=2e-5, err_msg=str(tag))
                    assert _rel_err(g, g_ref) < 2e-4, tag
                    assert _rel_err(g, gm0.cpu().numpy()) > 1e-2, tag


# ------------------------------------------------------------------------------------------------ 7. off is off


def test_off_is_off_and_on_is_deterministic(smpl, tables, dev):
    """Key absent == weight 0 == contacts None == all-zero contacts, bit for bit on loss and gradient, for the three closure
    kinds, on a fresh thread's workspace and on one that has just evaluated with the term on; F = 1 with the term on equals it
    too; two evaluations with the term on are bitwise equal."""
    F = 41
    seq, markers, o_pose, o_betas, root, trans, pert = _inputs(tables, F, 123)
    contacts = _contacts(F, 5)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, 5)
    absent = packaged_config("video_mocap")
    for k in ("chamfer", "marker"):
        assert "foot_lock" not in absent["stages"][k]["losses"]
    on = _cfg(W_CHAMFER, W_MARKER)
    for name, (make, pack) in _makers(smpl, dev, md, o_pose, o_betas, root, vids, i3, b3, pert).items():
        fresh = {}

        def on_fresh_thread():  # workspaces are per thread: this one has never seen the term
            p = make(absent, None)
            fresh["r"] = p.evaluate(pack(p), want_nn=False)[:2]
            torch.cuda.synchronize()

        t = threading.Thread(target=on_fresh_thread)
        t.start()
        t.join()
        pw = make(on, contacts)
        assert pw.foot_lock > 0.0
        x = pack(pw)
        lw, gw, _ = pw.evaluate(x, want_nn=False)       # the term on this thread's workspace first
        lw2, gw2, _ = pw.evaluate(x, want_nn=False)
        assert lw == lw2 and torch.equal(gw, gw2), name  # no float atomics
        lf, gf = fresh["r"]
        assert lw > lf and not torch.equal(gw, gf), name
        one = torch.zeros(F, 2)
        one[7, 0] = 1.0                                 # a one-frame contact: the gate is a product, nothing is gated
        variants = {"absent": (absent, contacts), "weight 0": (_cfg(0.0, 0.0), contacts), "no contacts": (on, None),
                    "zero contacts": (on, torch.zeros(F, 2)), "one-frame contact": (on, one)}
        for tag, (cfg, fc) in variants.items():
            p = make(cfg, fc)
            assert p.foot_lock == 0.0, (name, tag)
            pw.evaluate(x, want_nn=False)               # the workspace has just run with the term on
            l0, g0, _ = p.evaluate(x, want_nn=False)
            assert l0 == lf and torch.equal(g0, gf), (name, tag)

    # F = 1: no pair of frames, no term
    seq, markers, o_pose, o_betas, root, trans, pert = _inputs(tables, 1, 91)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, 6)
    for name, (make, pack) in _makers(smpl, dev, markers.to(dev), o_pose, o_betas, root, vids, i3, b3, pert).items():
        p1, p0 = make(on, torch.ones(1, 2)), make(absent, None)
        x = pack(p1)
        (l1, g1, _), (l0, g0, _) = p1.evaluate(x, want_nn=False), p0.evaluate(x, want_nn=False)
        assert l1 == l0 and torch.equal(g1, g0), name


# ------------------------------------------------------------------------------------------------ 8. compact packing
def test_third_rows_get_no_gradient_from_the_term(smpl, tables, dev):
    """The term reaches the raw rotations through the Gram-Schmidt backward only: with reg_pose_body 0 the third rows' gradient
    entries are exact zeros, and a solve on the compact packing leaves them bit for bit."""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    F = 37
    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, 111)
    contacts = _contacts(F, 8)
    md = markers.to(dev)
    cfg = _cfg(W_CHAMFER, W_MARKER)
    cfg["stages"]["chamfer"]["losses"]["reg_pose_body"] = 0.0
    cfg["stages"]["marker"]["losses"]["reg_pose_body"] = 0.0
    pc = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), cfg, foot_contacts=contacts)
    assert pc.foot_lock > 0
    x = pc.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    _, g, _ = pc.evaluate(x)
    gp = g[4 * F + 10:].reshape(F, 23, 3, 3)
    assert gp[:, :, :2].abs().sum() > 0 and not gp[:, :, 2].any()
    third = x[4 * F + 10:].reshape(F, 23, 3, 3)[:, :, 2].clone()
    pc.solve(x, max_iter=10, lr=0.1)
    assert torch.equal(x[4 * F + 10:].reshape(F, 23, 3, 3)[:, :, 2], third)

    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32).to(dev)
    pm = MarkerProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), vids, cfg, foot_contacts=contacts)
    xm = pm.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
    _, g, _ = pm.evaluate(xm)
    gp = g[:207 * F].reshape(F, 23, 3, 3)
    groot = g[207 * F + 10:216 * F + 10].reshape(F, 3, 3)
    assert gp[:, :, :2].abs().sum() > 0 and not gp[:, :, 2].any() and not groot[:, 2].any()
    third = xm[:207 * F].reshape(F, 23, 3, 3)[:, :, 2].clone()
    pm.solve(xm, max_iter=10, lr=1.0)
    assert torch.equal(xm[:207 * F].reshape(F, 23, 3, 3)[:, :, 2], third)


# ------------------------------------------------------------------------------------------------ 9. fused vs composed
def test_fused_and_composed_foot_lock_solves_agree(smpl, tables, dev):
    """25 L-BFGS iterations of the chamfer and the marker stage on the fused closures and on the operator-composed ones
    (execution.temporal_fused: False), with and without the robust data term: the start agrees to 1e-5, the end to 5e-2 / 8e-2
    (test_fused_and_composed_joint_accel_solves_agree's tolerances), and both decrease."""
    from uuo_mocap_amd.optimization import last_stats, optim_chamfer, optim_markers

    F = 37
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 121)
    contacts = _contacts(F, 9)
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
                          marker_labels=torch.zeros(F, M, dtype=torch.long, device=dev), smpl_inference=smpl, config=cfg,
                          foot_contacts=contacts)
            sc = dict(last_stats("chamfer"))
            o_pose_m = pose.detach().clone()
            optim_markers(md, pose_body=pose, o_pose_body=o_pose_m, betas=betas, o_betas=o_betas.to(dev), root_orient=rt,
                          trans=tr, barycentric_coords_one_hot=one_hot, img_mask=torch.ones(F, device=dev),
                          smpl_inference=smpl, config=cfg, foot_contacts=contacts)
            out[fused] = (sc, dict(last_stats("marker")))
        (cf, mf), (cc, mc) = out[True], out[False]
        assert "loss_first" in cc and "loss_first" in mc and "first_loss" in cf   # (the composed route's statistics)
        print("OBS foot_lock fused vs composed (sigma %g): chamfer %.6e -> %.6e / %.6e -> %.6e; marker %.6e -> %.6e / "
              "%.6e -> %.6e" % (sigma, first(cf), final(cf), first(cc), final(cc), first(mf), final(mf), first(mc), final(mc)))
        assert first(cf) == pytest.approx(first(cc), rel=1e-5)
        assert final(cf) == pytest.approx(final(cc), rel=5e-2)
        assert final(mf) == pytest.approx(final(mc), rel=8e-2)
        assert final(cf) < first(cf) and final(mf) < first(mf)


# ------------------------------------------------------------------------------------------------ 10. refusals and routing
def test_library_and_routes_refuse_the_term_where_it_is_not_built(smpl, tables, dev):
    from uuo_mocap_amd import parallel
    from uuo_mocap_amd.engine import ChamferProblem, PartProblem, solve_batch
    from uuo_mocap_amd.optimization import optim_chamfer, optim_markers

    F = 9
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 103)
    contacts = _contacts(F, 3)
    md = markers.to(dev)
    on = _cfg(W_CHAMFER, W_MARKER)
    # the library: part stage, bad weights, a weight without labels
    vlabels = torch.argmax(smpl.get_lbs_weights(), dim=-1)
    vidx = torch.cat([(vlabels == j).nonzero(as_tuple=True)[0] for j in (0, 1, 4, 7, 10)]).to(dev)
    pp = PartProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), vidx, packaged_config("video_mocap"))
    x = pp.pack(torch.zeros(1, 1, 1, device=dev), trans.to(dev), o_betas.to(dev))
    loss0 = pp.evaluate(x)[0]
    pp.foot_contacts = contacts.to(dev).contiguous()
    pp.foot_lock = 1.0  # what no config can produce: the library itself must refuse it
    with pytest.raises(RuntimeError, match="part stage"):
        pp.evaluate(x)
    pp.foot_lock = 0.0
    assert pp.evaluate(x)[0] == loss0
    lib = smpl.device_model.lib
    cptr = pp.foot_contacts.data_ptr()
    assert lib.uuo_fit_set_foot_lock(pp.fit, -1.0, cptr) != 0 and lib.uuo_fit_set_foot_lock(pp.fit, float("nan"), cptr) != 0
    assert lib.uuo_fit_set_foot_lock(pp.fit, float("inf"), cptr) != 0 and lib.uuo_fit_set_foot_lock(pp.fit, 1.0, None) != 0
    assert lib.uuo_fit_set_foot_lock(pp.fit, 0.0, None) == 0
    # lock-step batches
    p = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), on, foot_contacts=contacts)
    xc = p.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    with pytest.raises(NotImplementedError, match="lock-step"):
        solve_batch([p], [xc], max_iter=3)
    # frame-block sharding
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), vids.to(dev)] = 1.0
    pose, betas, rt, tr = (t.clone().to(dev) for t in (o_pose, o_betas, root, trans))
    with parallel.shard_frames(joint_with_one_rank=True):
        with pytest.raises(NotImplementedError, match="frame-block sharding"):
            optim_markers(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev), root_orient=rt,
                          trans=tr, barycentric_coords_one_hot=one_hot, img_mask=torch.ones(F, device=dev),
                          smpl_inference=smpl, config=on, foot_contacts=contacts)
        with pytest.raises(NotImplementedError, match="frame-block sharding"):
            optim_chamfer(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev),
                          root_orient=rt.reshape(F, 1, 3, 3), trans=tr, img_mask=torch.ones(F, device=dev),
                          marker_labels=torch.zeros(F, M, dtype=torch.long, device=dev), smpl_inference=smpl, config=on,
                          foot_contacts=contacts)


def _planted(tables, seed, F, markers):
    return make_sequence(tables, seed=seed, num_frames=F, num_markers=markers, planted_feet=True)


def test_lockstep_hypotheses_with_the_term_match_the_threaded_route(smpl, tables, dev):
    """hypothesis_lockstep: True cannot batch the term (lockstep_supported is False): the hypotheses run on threads and the
    fit is the threaded route's, bit for bit."""
    from uuo_mocap_amd.multimodal import multimodal_video_mocap

    seq = _planted(tables, 4, 24, 16)
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


# ------------------------------------------------------------------------------------------------ 11. what it buys


def _quality(out, seq, oracle_smpl):
    """(foot skate against the TRUE contacts in m/s, mean vertex error in m, acceleration error in m/s^2)"""
    from uuo_mocap_amd.metrics import compute_accel_error, compute_foot_skate

    r = oracle_smpl(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                    out["trans"].cpu().float())
    gt_j = torch.from_numpy(np.asarray(seq.gt["joints"]))[:, :24].float()
    true_c = torch.from_numpy(np.asarray(seq.gt["foot_contacts"]))
    return (float(compute_foot_skate(r["joints"][:, :24], true_c, 30.0)),
            float((r["vertices"] - torch.from_numpy(seq.gt["verts"])).norm(dim=-1).mean()),
            float(compute_accel_error(r["joints"][:, :24], gt_j, 30.0)))


def test_planted_feet_contact_config(smpl, oracle_smpl, tables, dev, record_property):
    """300 x 50 synthetic capture with planted feet (seed 0), once with all markers and once with the columns owned by joints
    7, 8, 10, 11 removed (M = 46), fitted with video_mocap.yaml and with video_mocap_contact.yaml.  Required: foot skate against
    the true contacts at most half the plain fit's on both captures, mean vertex error at most the plain fit's + 0.5 mm on
    both; and on a default (zero-contact) sequence video_mocap_contact.yaml gives the plain fit bit for bit.
    Measured with the shipped weights 0.3 / 0.1 (DESIGN.md section 4o has the sweep they were taken from): all markers -- foot
    skate 0.3677 m/s plain, 0.1689 m/s with the term (0.46 x), vertex error 6.70 / 6.65 mm, acceleration error 12.93 / 12.46
    m/s^2; without the foot and ankle markers -- 1.2095 / 0.3522 m/s (0.29 x), 8.69 / 8.29 mm, 17.93 / 15.66 m/s^2."""
    seq = _planted(tables, 0, 300, M)
    assert "foot_contacts" in seq.gt and float(seq.img_smpl.foot_contacts.sum()) > 0
    full = np.asarray(seq.markers.get_points()).copy()
    owner = np.argmax(np.asarray(tables.lbs_weights)[np.asarray(seq.gt["marker_vids"])], axis=1)
    keep = ~np.isin(owner, [7, 8, 10, 11])
    assert keep.sum() == 46
    res = {}
    for tag, pts in (("all", full), ("nofeet", full[:, keep])):
        for name in ("video_mocap", "video_mocap_contact"):
            res[(tag, name)] = _quality(_fit(seq, pts, name, smpl, dev), seq, oracle_smpl)
            for k, v in zip(("skate_mps", "vertex_m", "accel"), res[(tag, name)]):
                record_property("%s_%s_%s" % (tag, name, k), v)
        (s0, v0, a0), (s1, v1, a1) = res[(tag, "video_mocap")], res[(tag, "video_mocap_contact")]
        print("OBS planted feet (%s markers): foot skate plain %.4f contact %.4f m/s (%.2f x); vertex error plain %.2f contact "
              "%.2f mm; accel error plain %.3f contact %.3f m/s^2" % (tag, s0, s1, s1 / s0, 1e3 * v0, 1e3 * v1, a0, a1))
    for tag in ("all", "nofeet"):
        (s0, v0, _), (s1, v1, _) = res[(tag, "video_mocap")], res[(tag, "video_mocap_contact")]
        assert s1 <= 0.5 * s0, (tag, res)
        assert v1 <= v0 + 5e-4, (tag, res)

    # a capture without video contacts: the key changes nothing
    plain = make_sequence(tables, seed=3, num_frames=24, num_markers=16)
    assert not plain.img_smpl.foot_contacts.any()
    a, b = (_fit(plain, np.asarray(plain.markers.get_points()), n, smpl, dev, iters=30) for n in ("video_mocap", "video_mocap_contact"))
    for key in ("pose_body", "betas", "root_orient", "trans"):
        assert torch.equal(torch.as_tensor(a[key]), torch.as_tensor(b[key])), key
