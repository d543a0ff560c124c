"""EXTENSION: the 2D key-point reprojection term (stages.{chamfer,marker}.losses.keypoints_2d, uuo_fit_set_keypoints2d,
k_keypoint2d_fwd) on the MI355X -- the fused closures against float64 autograd, the term's gradient blocks, switched off, the
operator-composed route, the library's refusals, four evaluations in flight, the record's way through multimodal_video_mocap and
what video_mocap_keypoints.yaml buys on a capture whose HMR start has an elbow wrong in the image plane."""
import copy
import ctypes
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from capsules_ref64 import _caps_grad, _lists as _cap_lists, _preconditions as _caps_preconditions, _joints64  # noqa: E402
from floor_ref64 import _contacts, _planes, _vids  # noqa: E402
from gpu_support import (W_CAPS_C, W_CAPS_M, W_KP_C, W_KP_M, W_LIM_C, W_LIM_M, _inputs, _marker_x, _rel_err,  # noqa: E402,F401
                         _three_corners, dev, smpl, smpl64)
from joint_limits_ref64 import _lim_grad, _preconditions as _lim_preconditions, _tables as _lim_tables  # noqa: E402
from keypoints2d_ref64 import _kp_grad, _record, _with_key  # noqa: E402
from prior_confidence_ref64 import _cfg as _prior_cfg, _prior64, _weight_tables, _without  # noqa: E402
from stage_ref64 import (_chamfer_forward64, _float64, _marker_forward64, ref_chamfer64 as _ref_chamfer,  # noqa: E402
                         ref_marker64 as _ref_marker)
from uuo_mocap_amd.config import packaged_config  # noqa: E402

# W_KP_C, W_KP_M (0.05, 0.02), the weights of the parity checks, in pixels^-2: with targets 6 px of uniform noise off the projection, focal length 500 and four
# metres of depth a joint's gradient is 2 w c r f / (48 F p_z) ~ w 15 / F per component, a quarter of that under the Geman-McClure
# weights at sigma = 8 px.  The other terms at their parity weights (joint_accel 10, foot_lock 100, the capsules 100, the floor
# 100) bring the chamfer closure's float64 gradient to a norm of 10 and more, so 0.05 / 0.02 it is: the term's share of the
# float64 gradient is then past the 2e-2 that the precondition asks for in every case; asserted per case, before the comparison.
R_CHAMFER, R_MARKER = 1.0, 0.1   # video_mocap.yaml's reg_pose_body
SIGMA_KP = 8.0                   # pixels: of the residuals' own size, so that the Geman-McClure weights are far from 0 and 1
SHAPES = [(F, M) for F in (1, 2, 7, 33) for M in (10, 11)]
# seeds of the parity cases, chosen on the host: the first of 600 + 37 F + M + 1000 n (n = 0, 1, ...) that meets _check_seed
# and puts every joint at a depth >= 1 (n > 0: a foot's two lowest sole points within 1e-4 m at F = 7; at F = 33 a component of
# the +-0.2 rad table within 1e-4 rad of its hinge in one of the 33 x 69)
SEEDS = {(7, 11): 1870, (33, 10): 10831, (33, 11): 11832}

# the settings of the parity check: (name, the term's sigma, settings of test_gpu_prior_confidence's config, weighted prior)
SETTINGS = [
    ("plain", 0.0, {}, False),
    ("plain, sigma", SIGMA_KP, {}, False),
    ("capsules", 0.0, {"caps": True}, False),
    ("joint_accel + foot_lock", SIGMA_KP, {"temporal": True}, False),
    ("floor + offsets", 0.0, {"floor": True, "offs": True}, False),
    ("limits + prior weights", SIGMA_KP, {"limits": True}, True),
    ("robust_sigma", 0.0, {"sigma": 0.05}, False),
]


def _seed(F, M):
    return SEEDS.get((F, M), 600 + 37 * F + M)


def _check_seed(smpl64, tables, F, M, seed):
    """the float64 preconditions of the OTHER terms of the parity case (F, M, seed), host only: the +-0.2 rad limit table on the
    evaluated pose, the builder's capsule list (radii doubled) on both closures' joints, the floor planes (returned)"""
    pp = _inputs(tables, F, seed, num_markers=M)[6][3]
    lo, hi = _lim_tables()["full"]
    _lim_preconditions(pp, lo, hi, 3)
    for J in _joints64(smpl64, tables, F, M, seed):
        _caps_preconditions(J, _cap_lists(tables)["builder"], 1)
    return _planes(smpl64, tables, F, M, 6, seed)


def _compare(tag, loss, grad, l_rest, g_rest, l_kp, g_kp):
    lo, g_ref = l_rest + l_kp, g_rest + g_kp
    share = _rel_err(g_ref, g_rest)
    g = grad.cpu().numpy()
    print("OBS keypoints parity %s: loss rel %.2e, gradient rel %.2e, term's share of the gradient %.2e"
          % (tag, abs(loss - lo) / abs(lo), _rel_err(g, g_ref), share))
    assert share > 2e-2, ("the term's share of the float64 gradient is %.2e only" % share, tag)
    np.testing.assert_allclose(loss, lo, rtol=2e-5, err_msg=str(tag))
    assert _rel_err(g, g_ref) < 2e-4, tag


def _parity(smpl, smpl64, tables, dev, F, M, seed, alone=False):
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, seed, num_markers=M)
    contacts = _contacts(F, seed)
    svids = _vids(tables, 6)
    md = markers.to(dev)
    mvids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F, num_markers=M)
    args = (md, o_pose.to(dev), o_betas.to(dev))
    planes = _check_seed(smpl64, tables, F, M, seed)
    cap_list = _cap_lists(tables)["builder"]
    lim_tab = _lim_tables()["full"]
    wtab = _weight_tables(F, seed)["hash"]
    base = _prior_cfg(r_chamfer=R_CHAMFER, r_marker=R_MARKER)
    xc = ChamferProblem(smpl, *args, root.to(dev), base).pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))
    n0 = 219 * F + 10
    sl_c, sl_m = slice(4 * F + 10, 211 * F + 10), slice(0, 207 * F)
    forward_c = lambda: _chamfer_forward64(smpl64, xc.detach().cpu().double(), root.double(), F)
    with _float64():
        rec_c = _record(forward_c()[1]["joints"][:, :24].detach().numpy(), seed)
    rec_m = None
    for name, sigma_kp, kw, weighted in ([SETTINGS[0], SETTINGS[1]] if alone else SETTINGS):
        kw = dict(kw)
        offs = kw.pop("offs", False)
        if kw.get("floor"):
            kw["floor"] = planes
        if kw.get("caps"):
            kw["caps"] = cap_list
        limits = bool(kw.get("limits"))
        cfg0 = _prior_cfg(r_chamfer=R_CHAMFER, r_marker=R_MARKER, **kw)
        cfgm0 = _prior_cfg(r_chamfer=R_CHAMFER, r_marker=R_MARKER, offs=offs, **kw)
        if limits:   # (the +-0.2 rad table: active in every frame at every shape)
            for c in (cfg0, cfgm0):
                for stage in ("chamfer", "marker"):
                    c["stages"][stage]["joint_limits"] = {"lo": lim_tab[0].tolist(), "hi": lim_tab[1].tolist()}
        if alone:  # no data term, no priors: loss and gradient ARE the term
            for c in (cfg0, cfgm0):
                c["stages"]["chamfer"]["losses"].update(full_chamfer=0.0, reg_pose_body=0.0, reg_betas=0.0)
                c["stages"]["marker"]["losses"].update(marker=0.0, reg_pose_body=0.0, reg_betas=0.0)
        cfg, cfgm = _with_key(cfg0, W_KP_C, W_KP_M, sigma_kp), _with_key(cfgm0, W_KP_C, W_KP_M, sigma_kp)
        w = wtab if weighted else None
        reg_c, reg_m = (0.0, 0.0) if alone else (R_CHAMFER, R_MARKER)
        # ---- chamfer
        prob = ChamferProblem(smpl, *args, root.to(dev), cfg, foot_contacts=contacts, prior_weights=w, keypoints_2d=rec_c)
        prob0 = ChamferProblem(smpl, *args, root.to(dev), cfg0, foot_contacts=contacts, prior_weights=w)
        assert prob.keypoints_on and prob.kp_w == W_KP_C and prob.kp_sigma == sigma_kp and not prob0.keypoints_on
        assert prob.capsules_on == ("caps" in kw) and prob.joint_limits_on == limits and prob.prior_conf_on == weighted
        loss, grad, nn = prob.evaluate(xc)
        _, _, nn0 = prob0.evaluate(xc)
        assert torch.equal(nn, nn0), "the term must not change the assignment"
        l0, g0 = _ref_chamfer(smpl64, _without(cfg0), markers, o_pose, o_betas, root, xc, nn, contacts, svids, 3)
        with _float64():   # (a forward per setting: the terms' backward passes free its graph)
            leaves_c, out_c = forward_c()
        lk, gk = _kp_grad(leaves_c, out_c, rec_c, W_KP_C, sigma_kp)
        if "caps" in kw:
            lc, gc = _caps_grad(leaves_c, out_c, cap_list, W_CAPS_C)
            l0, g0 = l0 + lc, g0 + gc
        if limits:
            lt, gt = _lim_grad(leaves_c, 3, lim_tab, W_LIM_C)
            l0, g0 = l0 + lt, g0 + gt
        lp, gp = _prior64(xc, sl_c, o_pose, w, reg_c, g0.shape[0])
        _compare(("chamfer", name, F, M, alone), loss, grad, l0 + lp, g0 + gp, lk, gk)
        if alone:
            assert l0 + lp == 0.0 and not (g0 + gp).any()
        # ---- marker: one-hot and three-corner placements, with the latent offsets where the setting has them
        for assign, bary in ((mvids, None), (i3, b3)):
            mk = {"bary": None if bary is None else bary.to(dev), "foot_contacts": contacts, "prior_weights": w}
            pm0 = MarkerProblem(smpl, *args, assign.to(dev), cfgm0, **mk)
            xm = _marker_x(pm0, pp, bp, rp, tp, dev, F, num_markers=M)
            with _float64():
                leaves, out = _marker_forward64(smpl64, xm.detach().cpu().double()[:n0], F)
            if rec_m is None:   # (the first n0 entries of xm are the same for every marker closure of the case)
                rec_m = _record(out["joints"][:, :24].detach().numpy(), seed + 1)
            pm = MarkerProblem(smpl, *args, assign.to(dev), cfgm, keypoints_2d=rec_m, **mk)
            assert pm.keypoints_on and pm.kp_w == W_KP_M and not pm0.keypoints_on and pm.has_offsets == offs
            lm, gm, _ = pm.evaluate(xm, want_nn=False)
            l0, g0 = _ref_marker(smpl64, tables, _without(cfgm0), markers, o_pose, o_betas, xm, assign, bary, contacts, svids, 3, M)
            pad = 3 * M if offs else 0
            lk, gk = _kp_grad(leaves, out, rec_m, W_KP_M, sigma_kp, pad=pad)
            if "caps" in kw:
                lc, gc = _caps_grad(leaves, out, cap_list, W_CAPS_M, pad=pad)
                l0, g0 = l0 + lc, g0 + gc
            if limits:
                lt, gt = _lim_grad(leaves, 0, lim_tab, W_LIM_M, pad=pad)
                l0, g0 = l0 + lt, g0 + gt
            lp, gp = _prior64(xm, sl_m, o_pose, w, reg_m, g0.shape[0])
            tag = ("three-corner" if bary is not None else "one-hot", name, F, M, offs, alone)
            _compare(tag, lm, gm, l0 + lp, g0 + gp, lk, gk)


# ------------------------------------------------------------------------------------------------ 1. closure parity
@pytest.mark.parametrize("F,M", SHAPES)
def test_keypoint_closures_match_float64_autograd(smpl, smpl64, tables, dev, F, M):
    """Loss rtol 2e-5, gradient relative error < 2e-4 (test_gpu_capsules' tolerances) against float64 autograd: test_gpu_floor's
    restatement of the closures plus the capsules', the limit term's, the weighted prior's and the term's own
    (tests/keypoints2d_ref64.py), whose gradients add -- chamfer, one-hot and three-corner closures; the term with sigma 0 and 8 px;
    with the capsules (the kernel adds to their buffer), joint_accel + foot_lock, the floor term and the latent offsets, the
    joint-angle limits and a weighted prior, robust_sigma.  F = 1 and 7 leave the last block's upper half idle, F = 33 has 17
    blocks and an odd tail.  Asserted in float64 before anything is compared: the term's share of the gradient > 2e-2, every
    joint's depth >= 1, exact-zero confidences present and no other within 1e-4 of 0."""
    _parity(smpl, smpl64, tables, dev, F, M, _seed(F, M))


@pytest.mark.parametrize("F,M", [(1, 10), (2, 11), (7, 10), (33, 11)])
def test_the_term_alone_matches_float64(smpl, smpl64, tables, dev, F, M):
    """w_data = 0 and both priors 0: loss and gradient ARE the term, sigma 0 and 8 px (chamfer, one-hot and three-corner)."""
    _parity(smpl, smpl64, tables, dev, F, M, _seed(F, M), alone=True)


# ------------------------------------------------------------------------------------------------ helpers of 2 .. 7
def _case(smpl, smpl64, tables, dev, F, M, seed):
    """problem makers of one capture, its evaluated points and a record per stage, made from the float64 joints there"""
    from uuo_mocap_amd.engine import ChamferProblem, MarkerProblem

    seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, seed, num_markers=M)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
    i3, b3 = _three_corners(tables, seq, F, num_markers=M)
    a = (md, o_pose.to(dev), o_betas.to(dev))
    jc, jm = _joints64(smpl64, tables, F, M, seed)
    recs = {"chamfer": _record(jc, seed), "marker": _record(jm, seed + 1), "marker3": _record(jm, seed + 1)}
    makers = {
        "chamfer": (lambda c, **k: ChamferProblem(smpl, *a, root.to(dev), c, **k),
                    lambda p: p.pack(tp.to(dev), zp.to(dev), bp.to(dev), pp.to(dev))),
        "marker": (lambda c, **k: MarkerProblem(smpl, *a, vids.to(dev), c, **k),
                   lambda p: p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))),
        "marker3": (lambda c, **k: MarkerProblem(smpl, *a, i3.to(dev), c, bary=b3.to(dev), **k),
                    lambda p: p.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))),
    }
    return makers, recs


def _alone(cfg):
    cfg = copy.deepcopy(cfg)
    cfg["stages"]["chamfer"]["losses"].update(full_chamfer=0.0, reg_pose_body=0.0, reg_betas=0.0)
    cfg["stages"]["marker"]["losses"].update(marker=0.0, reg_pose_body=0.0, reg_betas=0.0)
    return cfg


# ------------------------------------------------------------------------------------------------ 2. the assignment
def test_the_term_changes_no_assignment(smpl, smpl64, tables, dev):
    """The nearest-vertex tables of the chamfer closure are equal with and without the term."""
    F, M = 7, 11
    makers, recs = _case(smpl, smpl64, tables, dev, F, M, 311)
    make, pack = makers["chamfer"]
    plain = packaged_config("video_mocap")
    p0, p1 = make(plain), make(_with_key(plain, 1.0, 1.0, SIGMA_KP), keypoints_2d=recs["chamfer"])
    assert p1.keypoints_on and not p0.keypoints_on
    x = pack(p0)
    l0, g0, nn0 = p0.evaluate(x)
    l1, g1, nn1 = p1.evaluate(x)
    assert torch.equal(nn0, nn1) and l1 > l0 and not torch.equal(g0, g1)


# ------------------------------------------------------------------------------------------------ 3. gradient blocks
def test_the_term_reaches_every_block_and_no_third_row(smpl, smpl64, tables, dev):
    """The term alone (no data term, no priors): its gradient reaches trans, betas, the root (z in the chamfer stage) and the
    body pose -- non-zero in every frame, and in every joint that has a child: a leaf's rotation moves none of the 24 joints,
    its rows are exact zeros -- and the third rows of the raw rotations receive exact zeros."""
    F, M = 7, 10
    makers, _ = _case(smpl, smpl64, tables, dev, F, M, 312)
    jc, jm = _joints64(smpl64, tables, F, M, 312)   # (every confidence positive: a zero on a hand would silence its wrist)
    recs = {"chamfer": _record(jc, 312, zero_every=0), "marker": _record(jm, 313, zero_every=0)}
    recs["marker3"] = recs["marker"]
    parents = [int(v) for v in tables.parents]
    inner = torch.tensor([j - 1 for j in range(1, 24) if j in parents], device=dev)
    leaf = torch.tensor([j - 1 for j in range(1, 24) if j not in parents], device=dev)
    assert len(leaf) == 5 and len(inner) == 18

    def pose_rows(g_pose):
        assert g_pose[:, inner, :2].abs().sum(dim=(2, 3)).min() > 0 and not g_pose[:, leaf].any() and not g_pose[:, :, 2].any()

    cfg = _alone(_with_key(packaged_config("video_mocap"), W_KP_C, W_KP_M, SIGMA_KP))
    pc = makers["chamfer"][0](cfg, keypoints_2d=recs["chamfer"])
    _, g, _ = pc.evaluate(makers["chamfer"][1](pc))
    g_trans, g_z, g_betas, g_pose = g[:3 * F], g[3 * F:4 * F], g[4 * F:4 * F + 10], g[4 * F + 10:].reshape(F, 23, 3, 3)
    assert g_trans.reshape(F, 3).abs().min() > 0 and g_z.abs().min() > 0 and g_betas.abs().min() > 0
    pose_rows(g_pose)
    for kind in ("marker", "marker3"):
        pm = makers[kind][0](cfg, keypoints_2d=recs[kind])
        _, g, _ = pm.evaluate(makers[kind][1](pm), want_nn=False)
        g_pose, g_betas = g[:207 * F].reshape(F, 23, 3, 3), g[207 * F:207 * F + 10]
        g_root, g_trans = g[207 * F + 10:216 * F + 10].reshape(F, 3, 3), g[216 * F + 10:219 * F + 10].reshape(F, 3)
        assert g_trans.abs().min() > 0 and g_betas.abs().min() > 0 and g_root[:, :2].abs().sum(dim=(1, 2)).min() > 0
        pose_rows(g_pose)
        assert not g_root[:, 2].any()


# ------------------------------------------------------------------------------------------------ 4. off is off
def test_off_is_off_and_on_is_deterministic(smpl, smpl64, tables, dev):
    """Key absent, weight 0, no record and all-zero confidences (also through joint weights) are bit-identical to the config
    without the key, on a workspace that has just run with the term on; two evaluations with the term on are bitwise equal; and a
    capsule closure evaluated after the term was armed and disarmed is bit-identical to what it was before the term was ever
    armed on its workspace: nothing leaks through the shared buffer."""
    F, M = 33, 11
    makers, recs = _case(smpl, smpl64, tables, dev, F, M, 313)
    absent = packaged_config("video_mocap")
    caps = _prior_cfg(r_chamfer=R_CHAMFER, r_marker=R_MARKER, caps=_cap_lists(tables)["builder"])
    for name, (make, pack) in makers.items():
        rec = recs[name]
        zero_conf = dict(rec, confidence=torch.zeros_like(rec["confidence"]))
        fresh = {}

        def on_fresh_thread():  # workspaces are per thread: this one has never seen the term
            p, pcap = make(absent), make(caps)
            fresh["plain"] = p.evaluate(pack(p), want_nn=False)[:2]
            fresh["caps"] = pcap.evaluate(pack(pcap), want_nn=False)[:2]
            torch.cuda.synchronize()

        t = threading.Thread(target=on_fresh_thread)
        t.start()
        t.join()
        on = _with_key(absent, W_KP_C, W_KP_M, SIGMA_KP)
        pw = make(on, keypoints_2d=rec)
        assert pw.keypoints_on
        x = pack(pw)
        lw, gw, _ = pw.evaluate(x, want_nn=False)
        lw2, gw2, _ = pw.evaluate(x, want_nn=False)
        assert lw == lw2 and torch.equal(gw, gw2), name  # no float atomics
        lf, gf = fresh["plain"]
        assert lw > lf and not torch.equal(gw, gf), name
        offs = {"absent": (absent, rec), "weight 0": (_with_key(absent, 0.0, 0.0, SIGMA_KP), rec), "no record": (on, None),
                "zero confidence": (on, zero_conf),
                "zero joint weights": (_with_key(absent, W_KP_C, W_KP_M, joint_weights=[0.0] * 24), rec),
                "key without block": (_with_key(absent, W_KP_C, W_KP_M, block=False), None)}
        for tag, (cfg, r) in offs.items():
            p = make(cfg, keypoints_2d=r)
            assert not p.keypoints_on, (name, tag)
            pw.evaluate(x, want_nn=False)               # the workspace has just run with the term on
            l0, g0, _ = p.evaluate(x, want_nn=False)
            assert l0 == lf and torch.equal(g0, gf), (name, tag)
        # the capsules' buffer: term + capsules, then the capsules alone
        both = make(_with_key(caps, W_KP_C, W_KP_M, SIGMA_KP), keypoints_2d=rec)
        assert both.keypoints_on and both.capsules_on
        lb, gb, _ = both.evaluate(x, want_nn=False)
        pcap = make(caps)
        lc, gc, _ = pcap.evaluate(x, want_nn=False)
        assert lc == fresh["caps"][0] and torch.equal(gc, fresh["caps"][1]), name
        assert lb > lc and not torch.equal(gb, gc), name
        lb2, gb2, _ = both.evaluate(x, want_nn=False)
        assert lb2 == lb and torch.equal(gb2, gb), name


# ------------------------------------------------------------------------------------------------ 5. fused vs composed
@pytest.mark.parametrize("F", [7, 33])
def test_fused_and_composed_keypoint_solves_agree(smpl, smpl64, tables, dev, F):
    """25 L-BFGS iterations of the chamfer and the marker stage on the fused closures and on the operator-composed ones
    (execution.keypoints_fused: False): the start agrees to 1e-5, the end to 5e-2 / 8e-2
    (test_fused_and_composed_capsule_solves_agree's tolerances), and both decrease."""
    from uuo_mocap_amd.optimization import last_stats, optim_chamfer, optim_markers

    M = 11
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 121 + F, num_markers=M)
    md = markers.to(dev)
    vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).long()
    one_hot = torch.zeros(M, smpl.device_model.V, device=dev)
    one_hot[torch.arange(M), vids.to(dev)] = 1.0
    with _float64(), torch.no_grad():   # targets: the start pose's joints, projected, with 6 px of noise
        x0 = torch.cat([o_pose.reshape(-1), o_betas.reshape(-1), root.reshape(-1), trans.reshape(-1)]).double()
        _, o0 = _marker_forward64(smpl64, x0, F)
    rec = _record(o0["joints"][:, :24].numpy(), 77 + F)
    first = lambda s: s.get("first_loss", s.get("loss_first"))
    final = lambda s: s.get("final_loss", s.get("loss_final"))
    out = {}
    for fused in (True, False):
        cfg = _with_key(packaged_config("video_mocap"), W_KP_C, W_KP_M, SIGMA_KP)
        cfg["execution"] = {"keypoints_fused": fused}
        for k in ("chamfer", "marker"):
            cfg["stages"][k]["num_iters"] = 25
        pose, betas, rt, tr = (t.clone().to(dev).requires_grad_(True) for t in (o_pose, o_betas, root, trans))
        optim_chamfer(md, pose_body=pose, o_pose_body=o_pose.to(dev), betas=betas, o_betas=o_betas.to(dev),
                      root_orient=rt, trans=tr, img_mask=torch.ones(F, device=dev),
                      marker_labels=torch.zeros(F, M, dtype=torch.long, device=dev), smpl_inference=smpl, config=cfg,
                      keypoints_2d=rec)
        sc = dict(last_stats("chamfer"))
        o_pose_m = pose.detach().clone()
        optim_markers(md, pose_body=pose, o_pose_body=o_pose_m, betas=betas, o_betas=o_betas.to(dev), root_orient=rt,
                      trans=tr, barycentric_coords_one_hot=one_hot, img_mask=torch.ones(F, device=dev),
                      smpl_inference=smpl, config=cfg, keypoints_2d=rec)
        out[fused] = (sc, dict(last_stats("marker")))
    (cf, mf), (cc, mc) = out[True], out[False]
    assert "loss_first" in cc and "loss_first" in mc and "first_loss" in cf   # (the composed route's statistics)
    print("OBS keypoints fused vs composed (F %d): chamfer %.6e -> %.6e / %.6e -> %.6e; marker %.6e -> %.6e / %.6e -> %.6e"
          % (F, first(cf), final(cf), first(cc), final(cc), first(mf), final(mf), first(mc), final(mc)))
    assert first(cf) == pytest.approx(first(cc), rel=1e-5)
    assert final(cf) == pytest.approx(final(cc), rel=5e-2)
    assert final(mf) == pytest.approx(final(mc), rel=8e-2)
    assert final(cf) < first(cf) and final(mf) < first(mf)
    assert final(cc) < first(cc) and final(mc) < first(mc)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_library_refuses_the_term_where_it_is_not_built(smpl, smpl64, tables, dev):
    from uuo_mocap_amd.engine import ChamferProblem, PartProblem, solve_batch

    F, M = 9, 11
    seq, markers, o_pose, o_betas, root, trans, _ = _inputs(tables, F, 103, num_markers=M)
    md = markers.to(dev)
    jc, _ = _joints64(smpl64, tables, F, M, 103)
    rec = _record(jc, 5)
    d = {k: v.to(dev).contiguous() for k, v in rec.items()}

    def arm(p, w=1.0):  # what no config can produce: the library itself must refuse it
        p.kp_cam, p.kp_targets, p.kp_conf, p.kp_w, p.kp_sigma, p.kp_min_depth = d["camera"], d["targets"], d["confidence"], w, 0.0, 0.1

    # the part stage refuses at evaluation
    vlabels = torch.argmax(smpl.get_lbs_weights(), dim=-1)
    vidx = torch.cat([(vlabels == j).nonzero(as_tuple=True)[0] for j in (0, 1, 4, 7, 10)]).to(dev)
    pp = PartProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), vidx, packaged_config("video_mocap"))
    x = pp.pack(torch.zeros(1, 1, 1, device=dev), trans.to(dev), o_betas.to(dev))
    loss0 = pp.evaluate(x)[0]
    arm(pp)
    with pytest.raises(RuntimeError, match="part stage"):
        pp.evaluate(x)
    arm(pp, 0.0)
    assert pp.evaluate(x)[0] == loss0
    # the soft chamfer closure refuses at evaluation
    soft = packaged_config("video_mocap")
    soft["stages"]["chamfer"]["losses"]["soft_chamfer"] = 10.0
    ps = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), soft)
    xs = ps.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    ls0 = ps.evaluate(xs)[0]
    arm(ps)
    with pytest.raises(RuntimeError, match="soft-assignment"):
        ps.evaluate(xs)
    arm(ps, 0.0)
    assert ps.evaluate(xs)[0] == ls0
    soft_on = _with_key(soft, 1.0, 1.0)
    with pytest.raises(NotImplementedError, match="soft-assignment closure"):
        ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), soft_on, keypoints_2d=rec)
    # the setter: every bad scalar and null array; off with null pointers
    lib, fit = smpl.device_model.lib, pp.fit
    cf = ctypes.c_float
    ptr = {k: v.data_ptr() for k, v in d.items()}

    def call(w=1.0, sigma=0.0, min_depth=0.1, cam=ptr["camera"], tg=ptr["targets"], cn=ptr["confidence"], fit=fit):
        return lib.uuo_fit_set_keypoints2d(fit, cf(w), cf(sigma), cf(min_depth), cam, tg, cn)

    assert call() == 0 and call(sigma=8.0) == 0
    assert call(fit=None) == -22
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert call(w=bad) == -22 and call(sigma=bad) == -22 and call(min_depth=bad) == -22, bad
    assert call(min_depth=0.0) == -22 and call(sigma=1e-30) == -22
    assert b"min_depth" in lib.uuo_last_error() or b"sigma" in lib.uuo_last_error()
    assert call(cam=None) == -22 and call(tg=None) == -22 and call(cn=None) == -22
    assert b"device" in lib.uuo_last_error()
    assert call(w=0.0, sigma=float("nan"), min_depth=-1.0, cam=None, tg=None, cn=None) == 0   # off: nothing else is looked at
    assert pp.evaluate(x)[0] == loss0
    # lock-step batches
    p = ChamferProblem(smpl, md, o_pose.to(dev), o_betas.to(dev), root.to(dev), _with_key(packaged_config("video_mocap"), 1.0, 1.0),
                       keypoints_2d=rec)
    assert p.keypoints_on
    xc = p.pack(trans.to(dev), torch.zeros(F, 1, 1, device=dev), o_betas.to(dev), o_pose.to(dev))
    with pytest.raises(NotImplementedError, match="lock-step.*keypoints_2d"):
        solve_batch([p], [xc], max_iter=3)


# ------------------------------------------------------------------------------------------------ 7. four in flight
def test_four_in_flight_are_bit_identical_to_one(smpl, smpl64, tables, dev):
    """parallel.fit_many over 8 marker-stage problems at F = 33, 30 evaluations each at perturbed points: every loss and
    gradient with inflight=4 is bitwise equal to the same work with inflight=1.  The marker closure runs neither k_skin3 nor the
    search: a difference can only come from k_keypoint2d_fwd or the backward."""
    from uuo_mocap_amd.engine import MarkerProblem
    from uuo_mocap_amd.parallel import fit_many

    F, M, N, E = 33, 11, 8, 30
    cfg = _with_key(packaged_config("video_mocap"), W_KP_C, W_KP_M, SIGMA_KP)
    items = []
    for i in range(N):
        seed = 400 + i
        seq, markers, o_pose, o_betas, root, trans, (tp, zp, bp, pp, rp) = _inputs(tables, F, seed, num_markers=M)
        _, jm = _joints64(smpl64, tables, F, M, seed)
        vids = torch.from_numpy(np.asarray(seq.gt["marker_vids"])).to(torch.int32)
        items.append((seed, markers, o_pose, o_betas, vids, (pp, bp, rp, tp), _record(jm, seed)))

    def work(item):
        seed, markers, o_pose, o_betas, vids, (pp, bp, rp, tp), rec = item
        pm = MarkerProblem(smpl, markers.to(dev), o_pose.to(dev), o_betas.to(dev), vids.to(dev), cfg, keypoints_2d=rec)
        assert pm.keypoints_on
        x0 = pm.pack(pp.to(dev), bp.to(dev), rp.to(dev), tp.to(dev))
        gen = torch.Generator().manual_seed(seed)
        out = []
        for e in range(E):
            x = (x0 + 0.01 * torch.randn(x0.numel(), generator=gen).to(dev)).contiguous()
            loss, grad, _ = pm.evaluate(x, want_nn=False)
            out.append((loss, grad.cpu()))
        return out

    one = fit_many(items, work, inflight=1, device=dev)
    four = fit_many(items, work, inflight=4, device=dev)
    wrong = [(i, e) for i in range(N) for e in range(E)
             if one[i][e][0] != four[i][e][0] or not torch.equal(one[i][e][1], four[i][e][1])]
    assert not wrong, "%d of %d evaluations differ with four in flight; the first: %s" % (len(wrong), N * E, wrong[:5])


# ------------------------------------------------------------------------------------------------ the pipeline's hook-up
def test_multimodal_hands_the_record_to_every_solve(smpl, dev, monkeypatch):
    """multimodal_video_mocap with the key on: every chamfer and marker solve, the final stage's included, receives the record --
    the explicit one cut and padded with the video's tracks (offset -2, 0, +2; the padded frames at confidence 0), also when
    the 2D-prior stage ran; without one, reprojection.world_keypoints_2d of the winning hypothesis when that stage ran, else
    none.  A record with another number of rows than the video, or beside differing frame rates, is refused."""
    import uuo_mocap_amd.multimodal as mm
    from uuo_mocap_amd.synthetic import SyntheticMarkers, make_sequence, synthetic_hmr_camera, synthetic_keypoints_2d

    F, M = 10, 12
    seq = make_sequence(smpl.tables, seed=6, num_frames=F, num_markers=M)
    seq.img_smpl.camera_bbox, seq.img_smpl.center, seq.img_smpl.size, seq.img_smpl.scale = synthetic_hmr_camera(F)
    rec = synthetic_keypoints_2d(seq, noise=1.0, seed=2)
    rec["confidence"] = rec["confidence"] * (0.5 + 0.05 * torch.arange(F, dtype=torch.float32))[:, None]   # every row its own
    calls = []

    def wrap(name, fn):
        def f(*a, **k):
            calls.append((name, k.get("repeat"), k.get("keypoints_2d")))
            return fn(*a, **k)
        return f

    monkeypatch.setattr(mm, "optim_chamfer", wrap("chamfer", mm.optim_chamfer))
    monkeypatch.setattr(mm, "optim_markers", wrap("marker", mm.optim_markers))

    def run(record, offset=0, reprojection=False, key=True, freq=30.0):
        cfg = _with_key(packaged_config("video_mocap"), 1e-5 if key else 0.0, 1e-6 if key else 0.0, 30.0)
        for k in ("part", "chamfer", "marker"):
            cfg["stages"][k]["num_iters"] = 4
        cfg["num_root_orient_angles"] = 2
        if reprojection:
            cfg["stages"]["reprojection_part"].update(num_iters=10, num_angles=2)
        del calls[:]
        out = mm.multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(np.asarray(seq.markers.get_points()).copy(), freq),
                                        dev, cfg, offset=offset, print_options=[], save_stages=False, smpl_inference=smpl,
                                        keypoints_2d=record)
        assert sorted((n, r) for n, r, _ in calls) == [("chamfer", 0), ("chamfer", 0), ("marker", 0), ("marker", 0), ("marker", 1)]
        assert all(torch.isfinite(out[k]).all() for k in ("trans", "pose_body", "root_orient", "betas"))
        return [r for _, _, r in calls], out

    for offset in (-2, 0, 2):
        got, out = run(rec, offset)
        n = abs(offset)
        assert out["trans"].shape[0] == F + n
        for r in got:
            assert {k: tuple(v.shape) for k, v in r.items()} == {"camera": (F + n, 16), "targets": (F + n, 24, 2), "confidence": (F + n, 24)}
            body = slice(n, None) if offset > 0 else slice(0, F)
            padded = slice(0, n) if offset > 0 else slice(F, None)
            edge = 0 if offset > 0 else F - 1
            for k in ("camera", "targets", "confidence"):
                assert torch.equal(r[k][body], rec[k]), (offset, k)
            assert not r["confidence"][padded].any() and r["confidence"][body].min() > 0
            for k in ("camera", "targets"):   # the padded rows repeat the edge row, as the video's tracks do
                assert torch.equal(r[k][padded], rec[k][[edge]].expand_as(r[k][padded])), (offset, k)
    # the 2D-prior stage ran: an explicit record still wins; without one the winning hypothesis is the record
    got, _ = run(rec, reprojection=True)
    assert all(torch.equal(r["targets"], rec["targets"]) for r in got)
    got, _ = run(None, reprojection=True)
    Ct = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0])
    for r in got:
        assert r["camera"].shape == (F, 16) and r["targets"].shape == (F, 24, 2) and r["confidence"].shape == (F, 24)
        assert torch.equal(r["camera"][:, :9], Ct[None].expand(F, 9)) and bool((r["camera"][:, 12:14] > 0).all())
        assert all(r[k] is got[0][k] or torch.equal(r[k], got[0][k]) for k in r)
    # neither: no record, and with the key off the 2D-prior stage's result is not even turned into one
    assert all(r is None for r in run(None)[0]) and all(r is None for r in run(None, reprojection=True, key=False)[0])
    with pytest.raises(ValueError, match="one row per video frame"):
        run({k: v[:F - 1] for k, v in rec.items()})
    with pytest.raises(NotImplementedError, match="frame rates"):
        run(rec, freq=60.0)


# ------------------------------------------------------------------------------------------------ 8. what it buys
def _fit_elbow(seq, cfg_name, rec, smpl, dev):
    from uuo_mocap_amd.multimodal import multimodal_video_mocap
    from uuo_mocap_amd.synthetic import SyntheticMarkers

    return multimodal_video_mocap(copy.deepcopy(seq.img_smpl), SyntheticMarkers(np.asarray(seq.markers.get_points()).copy(), 30.0),
                                  dev, packaged_config(cfg_name), offset=0, print_options=[], save_stages=False, smpl_inference=smpl,
                                  keypoints_2d=rec)


@pytest.mark.parametrize("seed", [0, 1])
def test_keypoints_config(smpl, oracle_smpl, tables, dev, record_property, seed):
    """video_mocap_keypoints.yaml on the sweep's capture (300 x 50, the HMR start's left forearm turned 0.5 rad in the image plane
    for 24 frames without arm markers; key points from the ground truth through a fixed camera, 2 px noise), on two seeds: the
    window's mean elbow and wrist error is lower than the plain fit's (video_mocap.yaml), and the vertex error is no more than
    0.5 mm above the plain fit's (test_capsules_config's margin).  Only the direction is asserted; the figures are recorded.
    Measured on an MI355X, on synthetic targets made from the ground truth: seed 0 window error 91.79 -> 33.18 mm,
    vertex 7.366 -> 6.758 mm; seed 1 window error 91.47 -> 60.76 mm, vertex 9.729 -> 9.277 mm."""
    from uuo_mocap_amd.synthetic import make_sequence, synthetic_keypoints_2d

    seq = make_sequence(tables, seed=seed, num_frames=300, num_markers=50, elbow_error=True)
    rec = synthetic_keypoints_2d(seq, noise=2.0, seed=seed)
    w0, w1 = seq.gt["elbow_window"]
    res = {}
    for name, r in (("video_mocap", None), ("video_mocap_keypoints", rec)):
        out = _fit_elbow(seq, name, r, smpl, dev)
        o = oracle_smpl(out["pose_body"].cpu().float(), out["betas"].cpu().float(), out["root_orient"].cpu().float(),
                        out["trans"].cpu().float())
        arm = float((o["joints"][w0:w1][:, [18, 20]] - torch.from_numpy(seq.gt["joints"])[w0:w1][:, [18, 20]]).norm(dim=-1).mean())
        verr = float((o["vertices"] - torch.from_numpy(seq.gt["verts"])).norm(dim=-1).mean())
        res[name] = (arm, verr)
        record_property("%s_window_elbow_wrist_mm" % name, 1e3 * arm)
        record_property("%s_vertex_mm" % name, 1e3 * verr)
    print("OBS keypoints config seed %d: window elbow + wrist %.2f -> %.2f mm, vertex %.3f -> %.3f mm"
          % (seed, 1e3 * res["video_mocap"][0], 1e3 * res["video_mocap_keypoints"][0], 1e3 * res["video_mocap"][1],
             1e3 * res["video_mocap_keypoints"][1]))
    assert res["video_mocap_keypoints"][0] < res["video_mocap"][0]
    assert res["video_mocap_keypoints"][1] <= res["video_mocap"][1] + 5e-4
